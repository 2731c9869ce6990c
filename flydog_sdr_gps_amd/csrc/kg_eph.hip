// kg_eph.hip -- ephemeris decode and satellite position and clock (kg_eph.h): EPHEM::Subframe, decode_page_e1b with its words,
// EPHEM::Page*, then SNAPSHOT::GetClock, GetClockCorrection, TimeOfEphemerisAge and GetXYZ per clock snapshot.
//
// A push runs two kernels over the rows kg_nav leaves in device memory:
//   fields  one lane per frame read: the payload unpacked, every raw field extracted and scaled (no state but the channel's kind)
//   walk    one lane per channel applies them in stream order: the channel's week_gst, the Page* "keep when 0" rules, notes, tow_bit
// and kg_eph_sv_dev one: one lane per snapshot.
#include "kg_common.h"
#include "kg_eph.h"

#include <new>
#include <vector>

using namespace kg_eph_cf;

static_assert(sizeof(ephem) == sizeof(kg_ephem) && sizeof(ephem) == 312 && offsetof(kg_ephem, tow_bit) == 304 && offsetof(ephem, tow_bit) == 304 &&
              offsetof(kg_ephem, kind) == offsetof(ephem, kind) && offsetof(kg_ephem, valid) == offsetof(ephem, valid) &&
              offsetof(kg_ephem, A_0G) == offsetof(ephem, A_0G) && offsetof(kg_ephem, alpha) == offsetof(ephem, alpha), "kg_ephem layout");
static_assert(sizeof(note) == sizeof(kg_eph_note) && sizeof(note) == 32 && offsetof(kg_eph_note, bit_next) == 24, "kg_eph_note layout");
static_assert(sizeof(snap) == sizeof(kg_eph_snap) && sizeof(snap) == 28 && sizeof(sv) == sizeof(kg_eph_pos) && sizeof(sv) == 48 &&
              offsetof(kg_eph_pos, flags) == 44, "snapshot layouts");
static_assert(KIND_NAVSTAR == KG_EPH_NAVSTAR && KIND_CA == KG_EPH_CA && KIND_E1B == KG_EPH_E1B && MAX_SATS == KG_EPH_MAX_SATS &&
              NAV_ERR_OOS == KG_NAV_ERR_OOS && SV_NOT_VALID == KG_EPH_SV_NOT_VALID && SV_POWER == KG_EPH_SV_POWER &&
              SV_TOW_DELAYED == KG_EPH_SV_TOW_DELAYED && SV_BAD == KG_EPH_SV_BAD && SV_TOO_OLD == KG_EPH_SV_TOO_OLD, "constants");
static_assert(sizeof(kg_nav_frame) == 64 && offsetof(kg_nav_frame, data) == 24, "kg_nav_frame layout");

struct eph_state { ephem slot[MAX_SATS]; chanst chan[KG_TRK_MAX_CHANS]; utc leap; };

__global__ void eph_zero_kernel(eph_state *st)
{
    uint32_t *w = reinterpret_cast<uint32_t *>(st);                     // one workgroup
    for (uint32_t i = threadIdx.x; i < sizeof(eph_state) / 4; i += blockDim.x) w[i] = 0;
    __syncthreads();
    if (threadIdx.x < KG_TRK_MAX_CHANS) st->chan[threadIdx.x].sat = -1;
}

// what: 0 bind channel ch to sat with kind (sat < 0: unbind), 1 clear slot sat, 2 clear channel ch's Galileo state
__global__ void eph_cmd_kernel(eph_state *st, int what, int ch, int sat, int kind)
{
    if (what == 0) {
        st->chan[ch].sat = sat; st->chan[ch].kind = kind;
        if (sat >= 0) {
            ephem e = st->slot[sat];
            e.kind = (uint32_t) kind;
            e.valid = valid(e);
            st->slot[sat] = e;
        }
    } else if (what == 1) {
        const uint32_t k = st->slot[sat].kind;
        uint32_t *w = reinterpret_cast<uint32_t *>(&st->slot[sat]);
        for (uint32_t i = 0; i < sizeof(ephem) / 4; i++) w[i] = 0;
        st->slot[sat].kind = k;
    } else {
        st->chan[ch].week_gst = 0; st->chan[ch].toes = 0; st->chan[ch].toc_gst = 0;
    }
}

__device__ inline int32_t row_count(const int32_t *counts, int ch, int cap)
{
    const int32_t n = counts[ch];
    return n < 0 ? 0 : (n > cap ? cap : n);
}

// fields: one lane per frame read
__global__ __launch_bounds__(64) void eph_fields_kernel(const eph_state *__restrict__ st, const kg_nav_frame *__restrict__ frames, size_t frame_stride,
                                                        const int32_t *__restrict__ counts, int cap, upd *__restrict__ ws, uint32_t ws_stride)
{
    const int ch = (int) blockIdx.y, k = (int) (blockIdx.x * 64 + threadIdx.x);
    if (k >= row_count(counts, ch, cap)) return;
    const kg_nav_frame *f = frames + (size_t) ch * frame_stride + k;
    upd o;
    fields(st->chan[ch].kind, f->err, f->data, o);
    ws[(size_t) ch * ws_stride + k] = o;
}

// walk: one lane per channel; two channels never share a satellite (kg_eph_set_sat), so the slots they write are apart
__global__ __launch_bounds__(64) void eph_walk_kernel(eph_state *__restrict__ st, int nchan, const kg_nav_frame *__restrict__ frames, size_t frame_stride,
                                                      const int32_t *__restrict__ counts, int cap, const upd *__restrict__ ws, uint32_t ws_stride,
                                                      note *__restrict__ notes, size_t note_stride)
{
    const int ch = (int) threadIdx.x;
    utc leap = {0, 0, 0, 0};
    int32_t has_leap = 0;
    if (ch < nchan) {
        chanst c = st->chan[ch];
        const int32_t n = row_count(counts, ch, cap);
        for (int32_t k = 0; k < n; k++) {
            const kg_nav_frame *f = frames + (size_t) ch * frame_stride + k;
            step(st->slot, c, ws[(size_t) ch * ws_stride + k], f->bit + (uint64_t) (int64_t) f->consumed, notes + (size_t) ch * note_stride + k, &leap,
                 &has_leap);
        }
        st->chan[ch] = c;
    }
    for (int c = 0; c < nchan; c++)                     // gps.delta_tLS / delta_tLSF / tLS_valid: channels in ascending order
        if (ch == c && has_leap) st->leap = leap;
}

// one lane per snapshot
__global__ __launch_bounds__(64) void eph_sv_kernel(const eph_state *__restrict__ st, const snap *__restrict__ snaps, int nsnap, sv *__restrict__ out)
{
    const int i = (int) (blockIdx.x * 64 + threadIdx.x);
    if (i >= nsnap) return;
    sv_one(st->slot, snaps[i], out + i);
}

struct kg_eph {
    kg_ctx *ctx;
    int nchan;
    std::vector<int> sat;               // the host's mirror of the bindings (-1: none)
    kg_dbuf<eph_state> d_st;
    kg_dbuf<upd> d_ws;                          // the field kernel's answers, ws_cap per channel
    int ws_cap;
};

// the workspace for pushes of up to cap frames per channel: grows, never shrinks
static int eph_reserve(kg_eph *v, int cap)
{
    if (cap <= v->ws_cap) return KG_OK;
    KG_HIP(hipStreamSynchronize(v->ctx->stream));                       // kernels of earlier pushes still use the old one
    v->d_ws.reset(); v->ws_cap = 0;
    const int c = (cap + 63) & ~63;
    KG_TRY(v->d_ws.alloc((size_t) c * v->nchan, "kg_eph: workspace"));
    v->ws_cap = c;
    return KG_OK;
}

static int eph_init(kg_eph *v)
{
    v->sat.assign(v->nchan, -1);
    int rc = v->d_st.alloc(1, "kg_eph_create: state");
    if (rc) return rc;
    hipLaunchKernelGGL(eph_zero_kernel, dim3(1), dim3(256), 0, v->ctx->stream, v->d_st.p);
    KG_TRY(eph_reserve(v, 64));
    KG_REQUIRE(hipGetLastError() == hipSuccess, KG_ERR_HIP, "kg_eph_create: launch failed");
    return KG_OK;
}

extern "C" {

int kg_eph_create(kg_ctx *ctx, int nchan, kg_eph **out)
{
    int rc = kg_ctx_use(ctx);
    if (rc) return rc;
    KG_REQUIRE(out != nullptr, KG_ERR_INVALID, "kg_eph_create: out is null");
    *out = nullptr;
    KG_REQUIRE(nchan >= 1 && nchan <= KG_TRK_MAX_CHANS, KG_ERR_INVALID, "kg_eph_create: nchan %d (1..%d)", nchan, KG_TRK_MAX_CHANS);
    kg_eph *v = new (std::nothrow) kg_eph();
    KG_REQUIRE(v != nullptr, KG_ERR_NOMEM, "kg_eph_create: alloc");
    v->ctx = ctx; v->nchan = nchan;
    rc = eph_init(v);
    if (rc) { kg_eph_destroy(v); return rc; }
    *out = v;
    return KG_OK;
}

void kg_eph_destroy(kg_eph *v) { kg_drain_delete(v); }

static int eph_cmd(kg_eph *v, int what, int ch, int sat, int kind)
{
    int rc = kg_ctx_use(v->ctx);
    if (rc) return rc;
    hipLaunchKernelGGL(eph_cmd_kernel, dim3(1), dim3(1), 0, v->ctx->stream, v->d_st, what, ch, sat, kind);
    KG_HIP(hipGetLastError());
    return KG_OK;
}

int kg_eph_set_sat(kg_eph *v, int ch, int sat, int kind)
{
    KG_REQUIRE(v != nullptr, KG_ERR_INVALID, "kg_eph_set_sat: null handle");
    KG_REQUIRE(ch >= 0 && ch < v->nchan, KG_ERR_INVALID, "kg_eph_set_sat: channel %d of %d", ch, v->nchan);
    KG_REQUIRE(sat >= -1 && sat < MAX_SATS, KG_ERR_INVALID, "kg_eph_set_sat: satellite %d (-1..%d)", sat, MAX_SATS - 1);
    KG_REQUIRE(kind == KG_EPH_NAVSTAR || kind == KG_EPH_CA || kind == KG_EPH_E1B, KG_ERR_INVALID, "kg_eph_set_sat: kind %d", kind);
    for (int c = 0; c < v->nchan; c++)
        KG_REQUIRE(sat < 0 || c == ch || v->sat[c] != sat, KG_ERR_INVALID, "kg_eph_set_sat: satellite %d is bound to channel %d", sat, c);
    int rc = eph_cmd(v, 0, ch, sat, kind);
    if (rc) return rc;
    v->sat[ch] = sat;
    return KG_OK;
}

int kg_eph_clear_sat(kg_eph *v, int sat)
{
    KG_REQUIRE(v != nullptr, KG_ERR_INVALID, "kg_eph_clear_sat: null handle");
    KG_REQUIRE(sat >= 0 && sat < MAX_SATS, KG_ERR_INVALID, "kg_eph_clear_sat: satellite %d (0..%d)", sat, MAX_SATS - 1);
    return eph_cmd(v, 1, 0, sat, 0);
}

int kg_eph_clear_chan(kg_eph *v, int ch)
{
    KG_REQUIRE(v != nullptr, KG_ERR_INVALID, "kg_eph_clear_chan: null handle");
    KG_REQUIRE(ch >= 0 && ch < v->nchan, KG_ERR_INVALID, "kg_eph_clear_chan: channel %d of %d", ch, v->nchan);
    return eph_cmd(v, 2, ch, 0, 0);
}

int kg_eph_push_frames_dev(kg_eph *v, const kg_nav_frame *d_frames, size_t frame_stride, const int32_t *d_counts, int cap, kg_eph_note *d_notes,
                           size_t note_stride)
{
    KG_REQUIRE(v && d_frames && d_counts && d_notes, KG_ERR_INVALID, "kg_eph_push_frames_dev: null argument");
    int rc = kg_ctx_use(v->ctx);
    if (rc) return rc;
    KG_REQUIRE(cap >= 0 && cap <= KG_NAV_MAX_PUSH, KG_ERR_INVALID, "kg_eph_push_frames_dev: cap %d outside 0..%d", cap, KG_NAV_MAX_PUSH);
    KG_REQUIRE((frame_stride >= (size_t) cap && note_stride >= (size_t) cap) || v->nchan == 1, KG_ERR_INVALID,
               "kg_eph_push_frames_dev: frame_stride %zu or note_stride %zu below cap %d", frame_stride, note_stride, cap);
    KG_REQUIRE(KG_ALIGNED(d_frames, 8) && KG_ALIGNED(d_counts, 4) && KG_ALIGNED(d_notes, 8), KG_ERR_INVALID,
               "kg_eph_push_frames_dev: d_frames and d_notes need 8-byte, d_counts 4-byte alignment");
    if (cap == 0) return KG_OK;
    rc = eph_reserve(v, cap);
    if (rc) return rc;
    hipStream_t s = v->ctx->stream;
    hipLaunchKernelGGL(eph_fields_kernel, dim3((unsigned) ((cap + 63) / 64), v->nchan), dim3(64), 0, s, (const eph_state *) v->d_st, d_frames, frame_stride,
                       d_counts, cap, v->d_ws, (uint32_t) v->ws_cap);
    hipLaunchKernelGGL(eph_walk_kernel, dim3(1), dim3(64), 0, s, v->d_st, v->nchan, d_frames, frame_stride, d_counts, cap, (const upd *) v->d_ws,
                       (uint32_t) v->ws_cap, (note *) d_notes, note_stride);
    KG_HIP(hipGetLastError());
    return KG_OK;
}

int kg_eph_push_frames(kg_eph *v, const kg_nav_frame *frames, size_t frame_stride, const int32_t *counts, int cap, kg_eph_note *notes, size_t note_stride)
{
    KG_REQUIRE(v && frames && counts && notes, KG_ERR_INVALID, "kg_eph_push_frames: null argument");
    int rc = kg_ctx_use(v->ctx);
    if (rc) return rc;
    KG_REQUIRE(cap >= 0 && cap <= KG_NAV_MAX_PUSH, KG_ERR_INVALID, "kg_eph_push_frames: cap %d outside 0..%d", cap, KG_NAV_MAX_PUSH);
    KG_REQUIRE((frame_stride >= (size_t) cap && note_stride >= (size_t) cap) || v->nchan == 1, KG_ERR_INVALID,
               "kg_eph_push_frames: frame_stride %zu or note_stride %zu below cap %d", frame_stride, note_stride, cap);
    std::vector<int32_t> n(v->nchan);
    for (int ch = 0; ch < v->nchan; ch++) n[ch] = counts[ch] < 0 ? 0 : (counts[ch] > cap ? cap : counts[ch]);
    const size_t rows = (size_t) v->nchan, least = cap ? (size_t) cap : 1;          // one channel: the strides are free, the device rows still hold cap
    const size_t fs = frame_stride > least ? frame_stride : least, ns = note_stride > least ? note_stride : least;
    kg_nav_frame *d_fr = nullptr;
    kg_eph_note *d_no = nullptr;
    int32_t *d_cnt = nullptr;
    hipStream_t s = v->ctx->stream;
    kg_scope tmp(v->ctx);                               // n[] and the device buffers are in use until it has drained the stream
    KG_TRY(tmp.alloc(&d_fr, fs * rows, "kg_eph_push_frames: frames"));
    KG_TRY(tmp.alloc(&d_no, ns * rows, "kg_eph_push_frames: notes"));
    KG_TRY(tmp.alloc(&d_cnt, rows, "kg_eph_push_frames: counts"));
    KG_HIP(hipMemcpyAsync(d_cnt, n.data(), sizeof(int32_t) * rows, hipMemcpyHostToDevice, s));
    for (int ch = 0; ch < v->nchan; ch++)
        if (n[ch]) KG_HIP(hipMemcpyAsync(d_fr + (size_t) ch * fs, frames + (size_t) ch * frame_stride, sizeof(kg_nav_frame) * n[ch], hipMemcpyHostToDevice, s));
    KG_TRY(kg_eph_push_frames_dev(v, d_fr, fs, d_cnt, cap, d_no, ns));
    for (int ch = 0; ch < v->nchan; ch++)
        if (n[ch]) KG_HIP(hipMemcpyAsync(notes + (size_t) ch * note_stride, d_no + (size_t) ch * ns, sizeof(kg_eph_note) * n[ch], hipMemcpyDeviceToHost, s));
    return KG_OK;                                       // tmp drains the stream: `notes` is filled when the caller sees it
}

int kg_eph_get(kg_eph *v, int sat, kg_ephem *out)
{
    KG_REQUIRE(v != nullptr && out != nullptr, KG_ERR_INVALID, "kg_eph_get: null argument");
    KG_REQUIRE(sat >= 0 && sat < MAX_SATS, KG_ERR_INVALID, "kg_eph_get: satellite %d (0..%d)", sat, MAX_SATS - 1);
    int rc = kg_ctx_use(v->ctx);
    if (rc) return rc;
    KG_HIP(hipMemcpyAsync(out, &v->d_st->slot[sat], sizeof(kg_ephem), hipMemcpyDeviceToHost, v->ctx->stream));
    KG_HIP(hipStreamSynchronize(v->ctx->stream));
    return KG_OK;
}

int kg_eph_get_chan(kg_eph *v, int ch, int32_t *sat, uint32_t *gst3)
{
    KG_REQUIRE(v && sat && gst3, KG_ERR_INVALID, "kg_eph_get_chan: null argument");
    KG_REQUIRE(ch >= 0 && ch < v->nchan, KG_ERR_INVALID, "kg_eph_get_chan: channel %d of %d", ch, v->nchan);
    int rc = kg_ctx_use(v->ctx);
    if (rc) return rc;
    chanst c;
    KG_HIP(hipMemcpyAsync(&c, &v->d_st->chan[ch], sizeof c, hipMemcpyDeviceToHost, v->ctx->stream));
    KG_HIP(hipStreamSynchronize(v->ctx->stream));
    *sat = c.sat; gst3[0] = c.week_gst; gst3[1] = c.toes; gst3[2] = c.toc_gst;
    return KG_OK;
}

int kg_eph_get_utc(kg_eph *v, int32_t *utc3)
{
    KG_REQUIRE(v && utc3, KG_ERR_INVALID, "kg_eph_get_utc: null argument");
    int rc = kg_ctx_use(v->ctx);
    if (rc) return rc;
    utc u;
    KG_HIP(hipMemcpyAsync(&u, &v->d_st->leap, sizeof u, hipMemcpyDeviceToHost, v->ctx->stream));
    KG_HIP(hipStreamSynchronize(v->ctx->stream));
    utc3[0] = u.delta_tLS; utc3[1] = u.delta_tLSF; utc3[2] = u.tLS_valid;
    return KG_OK;
}

int kg_eph_sv_dev(kg_eph *v, const kg_eph_snap *d_snaps, int nsnap, kg_eph_pos *d_out)
{
    KG_REQUIRE(v && d_snaps && d_out, KG_ERR_INVALID, "kg_eph_sv_dev: null argument");
    KG_REQUIRE(nsnap >= 0 && nsnap <= (1 << 24), KG_ERR_INVALID, "kg_eph_sv_dev: nsnap %d outside 0..%d", nsnap, 1 << 24);
    KG_REQUIRE(KG_ALIGNED(d_snaps, 4) && KG_ALIGNED(d_out, 8), KG_ERR_INVALID, "kg_eph_sv_dev: d_snaps needs 4-byte, d_out 8-byte alignment");
    int rc = kg_ctx_use(v->ctx);
    if (rc) return rc;
    if (nsnap == 0) return KG_OK;
    hipLaunchKernelGGL(eph_sv_kernel, dim3((unsigned) ((nsnap + 63) / 64)), dim3(64), 0, v->ctx->stream, (const eph_state *) v->d_st, (const snap *) d_snaps,
                       nsnap, (sv *) d_out);
    KG_HIP(hipGetLastError());
    return KG_OK;
}

int kg_eph_sv(kg_eph *v, const kg_eph_snap *snaps, int nsnap, kg_eph_pos *out)
{
    KG_REQUIRE(v && snaps && out, KG_ERR_INVALID, "kg_eph_sv: null argument");
    KG_REQUIRE(nsnap >= 0 && nsnap <= (1 << 24), KG_ERR_INVALID, "kg_eph_sv: nsnap %d outside 0..%d", nsnap, 1 << 24);
    int rc = kg_ctx_use(v->ctx);
    if (rc) return rc;
    if (nsnap == 0) return KG_OK;
    kg_eph_snap *d_in = nullptr;
    kg_eph_pos *d_o = nullptr;
    hipStream_t s = v->ctx->stream;
    kg_scope tmp(v->ctx);
    KG_TRY(tmp.alloc(&d_in, nsnap, "kg_eph_sv: snapshots"));
    KG_TRY(tmp.alloc(&d_o, nsnap, "kg_eph_sv: rows"));
    KG_HIP(hipMemcpyAsync(d_in, snaps, sizeof(kg_eph_snap) * nsnap, hipMemcpyHostToDevice, s));
    KG_HIP(hipMemcpyAsync(d_o, out, sizeof(kg_eph_pos) * nsnap, hipMemcpyHostToDevice, s));      // a refused snapshot keeps its row's values
    KG_TRY(kg_eph_sv_dev(v, d_in, nsnap, d_o));
    KG_HIP(hipMemcpyAsync(out, d_o, sizeof(kg_eph_pos) * nsnap, hipMemcpyDeviceToHost, s));
    return KG_OK;                                       // tmp drains the stream: `out` is filled when the caller sees it
}

void kg_eph_replica(uint32_t word, int32_t *chips, int32_t *cg_phase)
{
    int32_t c = 0, p = 0;
    replica_split(word, &c, &p);
    if (chips) *chips = c;
    if (cg_phase) *cg_phase = p;
}

}  // extern "C"
