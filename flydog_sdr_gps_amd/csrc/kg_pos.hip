// kg_pos.hip -- the position fix on the device (include/kiwigpu.h, kg_pos_*).  The arithmetic is csrc/kg_pos.h, shared
// with tools/pos_host_driver.cpp.  kg_pos_solve_dev is ONE launch of three single-wave workgroups, one per solver of SolveTask (all
// satellites, not Galileo, only Galileo): they share nothing but the compacted epoch, which each forms itself, and walk the call's
// epochs in order with their solver's state and every indexed matrix in LDS.  No barrier between workgroups, no atomics.
#include <memory>
#include <new>

#include "kg_common.h"
#include "kg_pos.h"

using namespace kg_pos_cf;

static_assert(sizeof(snap) == sizeof(kg_eph_snap) && sizeof(svrow) == sizeof(kg_eph_pos), "kg_pos.h mirrors kiwigpu.h");
static_assert(sizeof(fix) == sizeof(kg_pos_fix) && sizeof(satrec) == sizeof(kg_pos_sat) && sizeof(epoch_out) == sizeof(kg_pos_epoch) &&
              sizeof(solver) == sizeof(kg_pos_state), "kg_pos.h mirrors kiwigpu.h");
static_assert(sizeof(kg_pos_fix) == 80 && sizeof(kg_pos_sat) == 40 && sizeof(kg_pos_epoch) == 736 && sizeof(kg_pos_state) == 536, "the ABI's sizes");
static_assert(MAXN == KG_TRK_MAX_CHANS && MAX_SATS == KG_EPH_MAX_SATS && KIND_E1B == KG_EPH_E1B && SV_NOT_VALID == KG_EPH_SV_NOT_VALID &&
              SV_POWER == KG_EPH_SV_POWER && F_CALLED == KG_POS_CALLED && F_EKF_VALID == KG_POS_EKF_VALID, "kg_pos.h mirrors kiwigpu.h");

struct pos_state {
    solver s[3];
    int32_t kinds[MAX_SATS];
    int32_t use_kalman, plot_e1b;
    double uere, f_osc;
};

// what == 0: three fresh solvers; what == 1: the mode.  One lane.
__global__ void pos_cmd_kernel(pos_state *st, int what, int use_kalman, int plot_e1b)
{
    if (what == 0)
        for (int k = 0; k < 3; k++) solver_init(st->s[k]);
    else {
        st->use_kalman = use_kalman; st->plot_e1b = plot_e1b;
    }
}

// workgroup `which` = solver `which`, one wave
__global__ __launch_bounds__(64) void pos_solve_kernel(pos_state *__restrict__ st, const snap *__restrict__ snaps, const svrow *__restrict__ rows, int nrow,
                                                       int nepoch, const uint64_t *__restrict__ ticks, const uint32_t *__restrict__ skip,
                                                       epoch_out *__restrict__ out)
{
    __shared__ ws w;
    __shared__ epoch_in ep;
    const int which = (int) blockIdx.x, lane = (int) threadIdx.x;
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(&st->s[which]);
        uint32_t *dst = reinterpret_cast<uint32_t *>(&w.S);
        for (uint32_t i = threadIdx.x; i < sizeof(solver) / 4; i += 64) dst[i] = src[i];
    }
    const int use_kalman = st->use_kalman, plot_e1b = st->plot_e1b;
    const double uere = st->uere, f_osc = st->f_osc;
    __syncthreads();
    for (int e = 0; e < nepoch; e++) {
        if (lane == 0) load_epoch(ep, snaps + (size_t) e * nrow, rows + (size_t) e * nrow, nrow, skip ? skip[e] : 0u, st->kinds);
        __syncthreads();
        epoch_step(w, ep, which, use_kalman, plot_e1b, uere, f_osc, ticks[e], out + e, lane, 64);
        __syncthreads();
    }
    {
        uint32_t *dst = reinterpret_cast<uint32_t *>(&st->s[which]);
        const uint32_t *src = reinterpret_cast<const uint32_t *>(&w.S);
        for (uint32_t i = threadIdx.x; i < sizeof(solver) / 4; i += 64) dst[i] = src[i];
    }
}

struct kg_pos {
    kg_ctx *ctx;
    kg_dbuf<pos_state> d_st;
};

static int pos_cmd(kg_pos *v, int what, int use_kalman, int plot_e1b)
{
    int rc = kg_ctx_use(v->ctx);
    if (rc) return rc;
    hipLaunchKernelGGL(pos_cmd_kernel, dim3(1), dim3(1), 0, v->ctx->stream, v->d_st, what, use_kalman, plot_e1b);
    KG_HIP(hipGetLastError());
    return KG_OK;
}

static int pos_init(kg_pos *v, const int32_t kinds[64], double uere, double f_osc)
{
    std::unique_ptr<pos_state> h(new (std::nothrow) pos_state());
    KG_REQUIRE(h != nullptr, KG_ERR_NOMEM, "kg_pos_create: alloc");
    for (int k = 0; k < 3; k++) solver_init(h->s[k]);
    for (int k = 0; k < MAX_SATS; k++) h->kinds[k] = kinds[k];
    h->use_kalman = 1; h->plot_e1b = 0; h->uere = uere; h->f_osc = f_osc;
    KG_TRY(v->d_st.alloc(1, "kg_pos_create: state"));
    kg_scope tmp(v->ctx);                           // h is in use until the stream has drained
    KG_HIP(hipMemcpyAsync(v->d_st, h.get(), sizeof(pos_state), hipMemcpyHostToDevice, v->ctx->stream));
    KG_HIP(hipStreamSynchronize(v->ctx->stream));
    return KG_OK;
}

extern "C" {

int kg_pos_create(kg_ctx *ctx, const int32_t kinds[64], double uere, double f_osc, kg_pos **out)
{
    int rc = kg_ctx_use(ctx);
    if (rc) return rc;
    KG_REQUIRE(out != nullptr, KG_ERR_INVALID, "kg_pos_create: out is null");
    *out = nullptr;
    KG_REQUIRE(kinds != nullptr, KG_ERR_INVALID, "kg_pos_create: kinds is null");
    for (int k = 0; k < MAX_SATS; k++)
        KG_REQUIRE(kinds[k] == KG_EPH_NAVSTAR || kinds[k] == KG_EPH_CA || kinds[k] == KG_EPH_E1B, KG_ERR_INVALID, "kg_pos_create: kinds[%d] = %d", k, kinds[k]);
    KG_REQUIRE(uere > 0 && uere < 1e300 && f_osc > 0 && f_osc < 1e300, KG_ERR_INVALID, "kg_pos_create: uere %g and f_osc %g must be finite and positive", uere,
               f_osc);
    kg_pos *v = new (std::nothrow) kg_pos();
    KG_REQUIRE(v != nullptr, KG_ERR_NOMEM, "kg_pos_create: alloc");
    v->ctx = ctx;
    rc = pos_init(v, kinds, uere, f_osc);
    if (rc) { kg_pos_destroy(v); return rc; }
    *out = v;
    return KG_OK;
}

void kg_pos_destroy(kg_pos *v) { kg_drain_delete(v); }

int kg_pos_set_mode(kg_pos *v, int use_kalman, int plot_e1b)
{
    KG_REQUIRE(v != nullptr, KG_ERR_INVALID, "kg_pos_set_mode: null handle");
    KG_REQUIRE((use_kalman == 0 || use_kalman == 1) && (plot_e1b == 0 || plot_e1b == 1), KG_ERR_INVALID, "kg_pos_set_mode: use_kalman %d, plot_e1b %d (0 or 1)",
               use_kalman, plot_e1b);
    return pos_cmd(v, 1, use_kalman, plot_e1b);
}

int kg_pos_reset(kg_pos *v)
{
    KG_REQUIRE(v != nullptr, KG_ERR_INVALID, "kg_pos_reset: null handle");
    return pos_cmd(v, 0, 0, 0);
}

int kg_pos_solve_dev(kg_pos *v, const kg_eph_snap *d_snaps, const kg_eph_pos *d_sv, int nrow, int nepoch, const uint64_t *d_ticks, const uint32_t *d_skip,
                     kg_pos_epoch *d_out)
{
    KG_REQUIRE(v && d_snaps && d_sv && d_ticks && d_out, KG_ERR_INVALID, "kg_pos_solve_dev: null argument");
    KG_REQUIRE(nrow >= 1 && nrow <= KG_TRK_MAX_CHANS, KG_ERR_INVALID, "kg_pos_solve_dev: nrow %d (1..%d)", nrow, KG_TRK_MAX_CHANS);
    KG_REQUIRE(nepoch >= 1 && nepoch <= 65536, KG_ERR_INVALID, "kg_pos_solve_dev: nepoch %d (1..65536)", nepoch);
    KG_REQUIRE(KG_ALIGNED(d_snaps, 4) && KG_ALIGNED(d_skip, 4) && KG_ALIGNED(d_sv, 8) && KG_ALIGNED(d_ticks, 8) && KG_ALIGNED(d_out, 8), KG_ERR_INVALID,
               "kg_pos_solve_dev: d_snaps and d_skip need 4-byte, d_sv, d_ticks and d_out 8-byte alignment");
    int rc = kg_ctx_use(v->ctx);
    if (rc) return rc;
    hipLaunchKernelGGL(pos_solve_kernel, dim3(3), dim3(64), 0, v->ctx->stream, v->d_st, (const snap *) d_snaps, (const svrow *) d_sv, nrow, nepoch, d_ticks,
                       d_skip, (epoch_out *) d_out);
    KG_HIP(hipGetLastError());
    return KG_OK;
}

int kg_pos_solve(kg_pos *v, const kg_eph_snap *snaps, const kg_eph_pos *sv, int nrow, int nepoch, const uint64_t *ticks, const uint32_t *skip,
                 kg_pos_epoch *out)
{
    KG_REQUIRE(v && snaps && sv && ticks && out, KG_ERR_INVALID, "kg_pos_solve: null argument");
    KG_REQUIRE(nrow >= 1 && nrow <= KG_TRK_MAX_CHANS, KG_ERR_INVALID, "kg_pos_solve: nrow %d (1..%d)", nrow, KG_TRK_MAX_CHANS);
    KG_REQUIRE(nepoch >= 1 && nepoch <= 65536, KG_ERR_INVALID, "kg_pos_solve: nepoch %d (1..65536)", nepoch);
    int rc = kg_ctx_use(v->ctx);
    if (rc) return rc;
    const size_t n = (size_t) nrow * nepoch;
    const size_t o_snap = 0, o_sv = (o_snap + sizeof(kg_eph_snap) * n + 7) & ~(size_t) 7, o_tk = o_sv + sizeof(kg_eph_pos) * n,
                 o_out = o_tk + sizeof(uint64_t) * nepoch, o_skip = o_out + sizeof(kg_pos_epoch) * nepoch, total = o_skip + sizeof(uint32_t) * nepoch;
    char *d = nullptr;
    hipStream_t s = v->ctx->stream;
    kg_scope tmp(v->ctx);
    KG_TRY(tmp.alloc(&d, total, "kg_pos_solve"));
    KG_HIP(hipMemcpyAsync(d + o_snap, snaps, sizeof(kg_eph_snap) * n, hipMemcpyHostToDevice, s));
    KG_HIP(hipMemcpyAsync(d + o_sv, sv, sizeof(kg_eph_pos) * n, hipMemcpyHostToDevice, s));
    KG_HIP(hipMemcpyAsync(d + o_tk, ticks, sizeof(uint64_t) * nepoch, hipMemcpyHostToDevice, s));
    if (skip) KG_HIP(hipMemcpyAsync(d + o_skip, skip, sizeof(uint32_t) * nepoch, hipMemcpyHostToDevice, s));
    rc = kg_pos_solve_dev(v, (const kg_eph_snap *) (d + o_snap), (const kg_eph_pos *) (d + o_sv), nrow, nepoch, (const uint64_t *) (d + o_tk),
                          skip ? (const uint32_t *) (d + o_skip) : nullptr, (kg_pos_epoch *) (d + o_out));
    if (rc) return rc;
    KG_HIP(hipMemcpyAsync(out, d + o_out, sizeof(kg_pos_epoch) * nepoch, hipMemcpyDeviceToHost, s));
    return KG_OK;                                   // tmp drains the stream: `out` is filled when the caller sees it
}

int kg_pos_get_state(kg_pos *v, int solver_index, kg_pos_state *out)
{
    KG_REQUIRE(v != nullptr && out != nullptr, KG_ERR_INVALID, "kg_pos_get_state: null argument");
    KG_REQUIRE(solver_index >= 0 && solver_index < 3, KG_ERR_INVALID, "kg_pos_get_state: solver %d (0..2)", solver_index);
    int rc = kg_ctx_use(v->ctx);
    if (rc) return rc;
    KG_HIP(hipMemcpyAsync(out, &v->d_st->s[solver_index], sizeof(kg_pos_state), hipMemcpyDeviceToHost, v->ctx->stream));
    KG_HIP(hipStreamSynchronize(v->ctx->stream));
    return KG_OK;
}

}  // extern "C"
