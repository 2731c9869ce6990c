// kg_pos.h -- the arithmetic of the position fix: GNSSDataForEpoch::LoadFromReplicas' compaction (gps/solve.cpp:319-364), SolveTask's
// three solvers (solve.cpp:571-639), PosSolverImpl::solve (gps/PosSolver.cpp:64-144), SinglePointPositionSolver::Solve,
// EKFPositionSolver::update, PositionSolverBase::Iter / IterElevAzim, Ellipsoid::XYZ2LLH / dXYZdENU, TNT's matmult / mean / norm and JAMA's
// LU (pkgs/TNT_JAMA), and the az/el rule of update_gps_info_after (solve.cpp:497-516) -- for the device (kg_pos.hip) and, compiled by a
// host compiler, for tools/pos_host_driver.cpp, as kg_eph.h is.
//
// Every double is formed by the reference's operations in the reference's order, the zero terms of its dense products included (a NaN
// row makes every element of transpose(h) * weight * h NaN, as there); build without floating-point contraction.
//
// One code for both builds: every function takes (lane, nl).  The host calls with (0, 1).  On the device a solver is ONE wave: lane i
// does satellite i of the per-satellite stages and output element i, i + nl, ... of a product (the k loop inside an element stays the
// reference's), lane 0 does what is serial (the LU column recurrence, the state machine), and KG_POS_SYNC() -- a workgroup barrier, which
// a single-wave workgroup never waits at -- separates a stage from its readers.  Every branch around a stage reads its condition from the
// workspace after such a barrier, so the wave takes it as one.  Everything indexed lives in the workspace (LDS on the device).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KG_POS_FN __host__ __device__ static inline
#else
#define KG_POS_FN static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define KG_POS_SYNC() __syncthreads()
#else
#define KG_POS_SYNC() ((void) 0)
#endif

namespace kg_pos_cf {

enum { MAXN = 12,                                       // GPS_MAX_CHANS
       MAX_SATS = 64,
       SV_NOT_VALID = 1, SV_POWER = 2,                  // KG_EPH_SV_*
       KIND_E1B = 2,                                    // KG_EPH_E1B: the reference's `type == E1B`
       F_CALLED = 1, F_POS_VALID = 2, F_SPP_VALID = 4, F_EKF_VALID = 8,
       SPP_MAX_ITER = 20,                               // PosSolver.cpp:153, _spp(20, yield)
       LLH_MAX_ITER = 10 };                             // Ellipsoid.h:22

constexpr double C_LIGHT = 2.99792458e8;                // PositionSolverBase.h:27, _c
constexpr double OMEGA_E = 7.2921151467e-5;             // PositionSolverBase.h:26, _omega_e
constexpr double WGS84_A = 6378137.0;                   // Ellipsoid.h:20
constexpr double WGS84_B = 6356752.31424518;            // Ellipsoid.h:21
constexpr double LLH_DH = 1e-3;                         // Ellipsoid.h:23
constexpr double EKF_Q = 5e-5;                          // EKFPositionSolver.h:15, _q (all three)
constexpr double EKF_H0 = 1.8e-21, EKF_H1 = 6.5e-22, EKF_H2 = 1.4e-24;         // EKFPositionSolver.h:16, _h
constexpr double PI_M = 3.14159265358979323846;         // M_PI

struct snap { int32_t sat, bits, bits_tow, ms, chips, cg_phase; float power; };         // == kg_eph_snap
struct svrow { double x, y, z, ct, t_k; int32_t week, flags; };                         // == kg_eph_pos
struct fix { double x, y, z, t_rx, osc_corr, lambda, phi, alt; int32_t flags, ekf_running, nsv, pad; };          // == kg_pos_fix
struct satrec { double elev_deg, azim_deg; int32_t sat, ch, type, week, el, az; };      // == kg_pos_sat
struct epoch_out { fix f[3]; satrec sat[MAXN]; int32_t chans, grn_yel_red; uint32_t ch_has_soln, pad; };         // == kg_pos_epoch

struct solver {                                         // == kg_pos_state: PosSolverImpl's members with both solvers'
    double spp_state[4], spp_cov[16];                   // _spp._state, _spp._cov
    double ekf_state[5], ekf_P[25];                     // _ekf._state, _ekf._cov
    double pos[3], t_rx, osc_corr, lambda, phi, alt;    // _pos, _t_rx, _osc_corr, _llh
    double ct_rx[2];                                    // _ct_rx
    uint64_t ticks_spp[2], ticks_ekf[2];
    int32_t pos_valid, ekf_running, state_spp[2], ekf_valid, pad;       // ekf_valid: EKFPositionSolver::_valid
};

struct epoch_in {                                       // GNSSDataForEpoch after LoadFromReplicas
    int32_t chans, good;                                // good: LoadReplicas' count, the rows that were in Replicas
    double sv[4][MAXN], weight[MAXN];
    int32_t sat[MAXN], ch[MAXN], type[MAXN], week[MAXN];
};

struct ws {                                             // one solver's workspace
    solver S;
    int32_t nsv, n, ok, brk, run_ekf, sing, pivsign, pad_;
    double det, dt;
    double sv[4][MAXN], wgt[MAXN];                      // the solver's set; wgt is normalised in place, as `weight /=` does
    double W[MAXN * MAXN];                              // makeDiag(weight); R in the EKF
    double h[MAXN * 5], hT[5 * MAXN], dz[MAXN], wk[MAXN];
    double ch[MAXN * 3], cdz[MAXN];                     // the EKF's candidates before its outlier gate
    int32_t keep[MAXN];
    double A[MAXN * MAXN], B[MAXN * MAXN];              // products
    double M[MAXN * MAXN], LU[MAXN * MAXN], X[MAXN * MAXN], col[MAXN];
    int32_t piv[MAXN];
    double Phi[25], PhiT[25], Pp[25], Q[25], T1[25], T2[25], G[5 * MAXN];
    double xp[5], dx[5];
    double h3[9], h3T[9], q3[9], t3[9];
};

// ---- TNT
// matmult (tnt/array2d_utils.h:233): C (M x K) = A (M x N) * B (N x K), `sum = 0; sum += A[i][k] * B[k][j]`; one element per lane and turn
KG_POS_FN void mm_part(double *Cm, const double *A, const double *B, int M, int N, int K, int lane, int nl)
{
    for (int e = lane; e < M * K; e += nl) {
        const int i = e / K, j = e - i * K;
        double sum = 0;
        for (int k = 0; k < N; k++) sum += A[i * N + k] * B[k * K + j];
        Cm[e] = sum;
    }
}

KG_POS_FN void mm(double *Cm, const double *A, const double *B, int M, int N, int K, int lane, int nl)
{
    mm_part(Cm, A, B, M, N, K, lane, nl);
    KG_POS_SYNC();
}

KG_POS_FN void tr(double *T, const double *A, int M, int N, int lane, int nl)            // transpose: T (N x M) of A (M x N)
{
    for (int e = lane; e < M * N; e += nl) {
        const int i = e / N, j = e - i * N;
        T[j * M + i] = A[e];
    }
    KG_POS_SYNC();
}

KG_POS_FN double norm3(double a, double b, double c)    // TNT::norm: sum(0); sum += A[i] * A[i]; sqrt
{
    double sum = 0;
    sum += a * a; sum += b * b; sum += c * c;
    return sqrt(sum);
}

// makeDiag (tnt/utils.h:32), serial
KG_POS_FN void make_diag(double *D, const double *v, int n)
{
    for (int i = 0; i < n * n; i++) D[i] = 0;
    for (int i = 0; i < n; i++) D[i * n + i] = v[i];
}

// ---- JAMA::LU (jama/lu.h): the left-looking dot-product Crout / Doolittle with partial pivoting, det(); lane 0
KG_POS_FN void lu_factor(ws &w, const double *A, int n)
{
    double *LU = w.LU, *col = w.col;
    for (int i = 0; i < n * n; i++) LU[i] = A[i];
    for (int i = 0; i < n; i++) w.piv[i] = i;
    int pivsign = 1;
    for (int j = 0; j < n; j++) {
        for (int i = 0; i < n; i++) col[i] = LU[i * n + j];
        for (int i = 0; i < n; i++) {
            const int kmax = i < j ? i : j;
            double s = 0.0;
            for (int k = 0; k < kmax; k++) s += LU[i * n + k] * col[k];
            col[i] -= s;
            LU[i * n + j] = col[i];
        }
        int p = j;
        for (int i = j + 1; i < n; i++)
            if (fabs(col[i]) > fabs(col[p])) p = i;
        if (p != j) {
            for (int k = 0; k < n; k++) { const double t = LU[p * n + k]; LU[p * n + k] = LU[j * n + k]; LU[j * n + k] = t; }
            const int k = w.piv[p]; w.piv[p] = w.piv[j]; w.piv[j] = k;
            pivsign = -pivsign;
        }
        if (LU[j * n + j] != 0.0)
            for (int i = j + 1; i < n; i++) LU[i * n + j] /= LU[j * n + j];
    }
    double d = (double) pivsign;
    int sing = 0;
    for (int j = 0; j < n; j++) { d *= LU[j * n + j]; if (LU[j * n + j] == 0) sing = 1; }
    w.det = d; w.sing = sing; w.pivsign = pivsign;
}

// LU::solve(eye(n)): the columns of X are independent, one per lane; within a column the reference's k, i order
KG_POS_FN void lu_inverse(ws &w, int n, int lane, int nl)
{
    const double *LU = w.LU;
    double *X = w.X;
    for (int j = lane; j < n; j += nl) {
        for (int i = 0; i < n; i++) X[i * n + j] = w.piv[i] == j ? 1.0 : 0.0;
        for (int k = 0; k < n; k++)
            for (int i = k + 1; i < n; i++) X[i * n + j] -= X[k * n + j] * LU[i * n + k];
        for (int k = n - 1; k >= 0; k--) {
            X[k * n + j] /= LU[k * n + k];
            for (int i = 0; i < k; i++) X[i * n + j] -= X[k * n + j] * LU[i * n + k];
        }
    }
    KG_POS_SYNC();
}

// ---- PositionSolverBase
KG_POS_FN double mod_gpsweek_rel(double cdt)            // PositionSolverBase.h:73-79
{
    const double cws = C_LIGHT * 7 * 24 * 3600;
    cdt -= (cdt > +0.5 * cws) * cws;
    cdt += (cdt < -0.5 * cws) * cws;
    return cdt;
}

KG_POS_FN double mod_gpsweek_abs(double cdt)            // PositionSolverBase.h:81-87
{
    const double cws = C_LIGHT * 7 * 24 * 3600;
    cdt -= (cdt >= cws) * cws;
    cdt += (cdt < 0) * cws;
    return cdt;
}

// pos - MakeRotZ(theta) * satpos: the 3 x 3 by 3 x 1 matmult with its zero terms (PositionSolverBase.h:97-98, :102-105)
KG_POS_FN void rot_diff(double theta, double x, double y, double z, double px, double py, double pz, double *d0, double *d1, double *d2)
{
    const double ct = cos(theta), st = sin(theta);
    double s0 = 0, s1 = 0, s2 = 0;
    s0 += ct * x; s0 += -st * y; s0 += 0.0 * z;
    s1 += st * x; s1 += ct * y; s1 += 0.0 * z;
    s2 += 0.0 * x; s2 += 0.0 * y; s2 += 1.0 * z;
    *d0 = px - s0; *d1 = py - s1; *d2 = pz - s2;
}

// one satellite of Iter(ct_rx, sv, f) (PositionSolverBase.h:92-101)
KG_POS_FN void iter_sat(double ct_rx, double x, double y, double z, double ct_tx, double px, double py, double pz, double *d0, double *d1, double *d2,
                        double *cdt_out)
{
    const double cdt = mod_gpsweek_rel(ct_rx - ct_tx);
    const double theta = -cdt / C_LIGHT * OMEGA_E;
    rot_diff(theta, x, y, z, px, py, pz, d0, d1, d2);
    *cdt_out = cdt;
}

// ---- Ellipsoid
KG_POS_FN double wgs84_e2() { return 1.0 - (WGS84_B * WGS84_B) / (WGS84_A * WGS84_A); }

KG_POS_FN double phi_iter(double z_by_rho, double nu_ratio) { return atan(z_by_rho / (1.0 - wgs84_e2() * nu_ratio)); }

KG_POS_FN void xyz2llh(double x, double y, double z, double *lambda, double *phi_out, double *alt_out)          // Ellipsoid.h:39-54
{
    double sum = 0;
    sum += x * x; sum += y * y;
    const double rho = sqrt(sum);
    const double z_by_rho = z / rho;
    *lambda = 2.0 * atan2(y, x + rho);
    double alt0 = 0, alt1 = 0;
    double phi = phi_iter(z_by_rho, 1.0);
    for (int i = 0; i < LLH_MAX_ITER; ++i) {
        const double sp = sin(phi);
        const double nu = WGS84_A / sqrt(1.0 - wgs84_e2() * sp * sp);
        alt1 = rho / cos(phi) - nu;
        phi = phi_iter(z_by_rho, nu / (nu + alt1));
        if (fabs(alt1 - alt0) < LLH_DH) break;
        alt0 = alt1;
    }
    *phi_out = phi; *alt_out = alt1;
}

KG_POS_FN void dxyz_denu(double lambda, double phi, double *h)                          // Ellipsoid.h:57-63
{
    const double cp = cos(phi), sp = sin(phi);
    const double cl = cos(lambda), sl = sin(lambda);
    h[0] = -sl; h[1] = -sp * cl; h[2] = cp * cl;
    h[3] = +cl; h[4] = -sp * sl; h[5] = cp * sl;
    h[6] = 0.0; h[7] = +cp; h[8] = sp;
}

// ---- SinglePointPositionSolver
// ComputeCov (SinglePointPositionSolver.h:55-64): transpose(h) * weight * h left to right, invert_lu, det > 1e-20
KG_POS_FN bool spp_compute_cov(ws &w, int lane, int nl)
{
    const int n = w.nsv;
    tr(w.hT, w.h, n, 4, lane, nl);
    mm(w.A, w.hT, w.W, 4, n, n, lane, nl);
    mm(w.M, w.A, w.h, 4, n, 4, lane, nl);
    if (lane == 0) lu_factor(w, w.M, 4);
    KG_POS_SYNC();
    if (!w.sing) lu_inverse(w, 4, lane, nl);            // a singular LU::solve returns the 0 x 0 array: dim1() != 4
    if (lane == 0) {
        w.ok = !w.sing && w.det > 1e-20;
        if (w.ok)
            for (int i = 0; i < 16; i++) w.S.spp_cov[i] = w.X[i];
    }
    KG_POS_SYNC();
    return w.ok != 0;
}

KG_POS_FN bool spp_solve(ws &w, int lane, int nl)                                       // SinglePointPositionSolver.h:20-52
{
    const int n = w.nsv;
    solver &S = w.S;
    if (n < 4) return false;
    if (lane == 0) {
        double sum = 0;
        for (int i = 0; i < n; i++) sum += w.sv[3][i];
        const double ct0 = sum / (double) n + C_LIGHT * 75e-3;
        S.spp_state[0] = 0; S.spp_state[1] = 0; S.spp_state[2] = 0; S.spp_state[3] = ct0;
    }
    KG_POS_SYNC();
    int i = 0;
    for (; i < SPP_MAX_ITER; ++i) {
        for (int s = lane; s < n; s += nl) {
            double d0, d1, d2, cdt;
            iter_sat(S.spp_state[3], w.sv[0][s], w.sv[1][s], w.sv[2][s], w.sv[3][s], S.spp_state[0], S.spp_state[1], S.spp_state[2], &d0, &d1, &d2, &cdt);
            const double dpn = norm3(d0, d1, d2);
            w.h[s * 4 + 0] = d0 / dpn; w.h[s * 4 + 1] = d1 / dpn; w.h[s * 4 + 2] = d2 / dpn;
            w.h[s * 4 + 3] = -1;
            w.dz[s] = dpn - cdt;                        // drho
        }
        KG_POS_SYNC();
        if (!spp_compute_cov(w, lane, nl)) return false;
        mm(w.A, S.spp_cov, w.hT, 4, 4, n, lane, nl);    // cov() * transpose(h) * weight * drho, left to right
        mm(w.B, w.A, w.W, 4, n, n, lane, nl);
        if (lane == 0) {
            for (int r = 0; r < 4; r++) {
                double c = 0;
                for (int j = 0; j < n; j++) c += w.B[r * n + j] * w.dz[j];
                w.dx[r] = c;
            }
            for (int r = 0; r < 4; r++) S.spp_state[r] -= w.dx[r];
            S.spp_state[3] = mod_gpsweek_abs(S.spp_state[3]);
            w.brk = norm3(w.dx[0], w.dx[1], w.dx[2]) < 0.001;
        }
        KG_POS_SYNC();
        if (w.brk) break;
    }
    return i < SPP_MAX_ITER;
}

// ---- EKFPositionSolver
KG_POS_FN void ekf_make_q(ws &w, double dt)             // MakeQ (EKFPositionSolver.h:108-124); lane 0
{
    const solver &S = w.S;
    const double c2 = C_LIGHT * C_LIGHT;
    dt = 0.1 < dt ? dt : 0.1;                           // std::max(0.1, dt)
    const double dt2 = dt * dt;
    const double dt3 = dt2 * dt;
    double *q = w.Q;
    for (int i = 0; i < 25; i++) q[i] = 0.0;
    q[0] = EKF_Q * EKF_Q;                               // std::pow(_q[i], 2)
    q[6] = EKF_Q * EKF_Q;
    q[12] = EKF_Q * EKF_Q;
    q[18] = c2 * (0.5 * EKF_H0 * dt + 2 * EKF_H1 * dt2 + 2.0 / 3.0 * PI_M * PI_M * EKF_H2 * dt3);
    q[19] = q[23] = c2 * (2 * EKF_H1 * dt + PI_M * PI_M * EKF_H2 * dt2);
    q[24] = c2 * (0.5 * EKF_H0 / dt + 2 * EKF_H1 + 8.0 / 3.0 * PI_M * PI_M * EKF_H2 * dt);
    if (S.ekf_valid) {
        double lambda, phi, alt;
        xyz2llh(S.ekf_state[0], S.ekf_state[1], S.ekf_state[2], &lambda, &phi, &alt);
        dxyz_denu(lambda, phi, w.h3);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) { w.q3[i * 3 + j] = q[i * 5 + j]; w.h3T[j * 3 + i] = w.h3[i * 3 + j]; }
        mm_part(w.t3, w.h3, w.q3, 3, 3, 3, 0, 1);       // h * q(0:2, 0:2) * transpose(h); lane 0 alone, so without the barrier
        mm_part(w.q3, w.t3, w.h3T, 3, 3, 3, 0, 1);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) q[i * 5 + j] = w.q3[i * 3 + j];
    }
}

KG_POS_FN bool ekf_fail(ws &w, int lane)
{
    if (lane == 0) w.S.ekf_valid = 0;
    KG_POS_SYNC();
    return false;
}

KG_POS_FN bool ekf_update(ws &w, double dt, int lane, int nl)                           // EKFPositionSolver.h:28-100
{
    solver &S = w.S;
    const int n0 = w.nsv;
    if (n0 < 1) return ekf_fail(w, lane);
    if (lane == 0) {
        for (int i = 0; i < 25; i++) w.Phi[i] = 0;
        for (int i = 0; i < 5; i++) w.Phi[i * 5 + i] = 1;
        w.Phi[3 * 5 + 4] = dt;
        for (int i = 0; i < 5; i++) {
            double c = 0;
            for (int j = 0; j < 5; j++) c += w.Phi[i * 5 + j] * S.ekf_state[j];
            w.xp[i] = c;
        }
        w.xp[3] = mod_gpsweek_abs(w.xp[3]);
    }
    KG_POS_SYNC();
    for (int s = lane; s < n0; s += nl) {
        double d0, d1, d2, cdt;
        iter_sat(w.xp[3], w.sv[0][s], w.sv[1][s], w.sv[2][s], w.sv[3][s], S.ekf_state[0], S.ekf_state[1], S.ekf_state[2], &d0, &d1, &d2, &cdt);
        const double z = cdt;
        const double zp = norm3(d0, d1, d2);
        w.keep[s] = fabs(z - zp) < 1e3;
        w.cdz[s] = z - zp;
        w.ch[s * 3 + 0] = d0 / zp; w.ch[s * 3 + 1] = d1 / zp; w.ch[s * 3 + 2] = d2 / zp;
    }
    KG_POS_SYNC();
    if (lane == 0) {
        int n = 0;
        for (int s = 0; s < n0; s++)
            if (w.keep[s]) {
                w.dz[n] = w.cdz[s];
                w.h[n * 5 + 0] = w.ch[s * 3 + 0]; w.h[n * 5 + 1] = w.ch[s * 3 + 1]; w.h[n * 5 + 2] = w.ch[s * 3 + 2];
                w.h[n * 5 + 3] = -1;
                w.h[n * 5 + 4] = 0;
                w.wk[n] = w.wgt[n];                     // w(nsv) = weight(nsv): the COMPACTED index, as the reference has it
                ++n;
            }
        w.n = n;
        if (n >= 1) {
            make_diag(w.W, w.wk, n);                    // R
            ekf_make_q(w, dt);
        }
    }
    KG_POS_SYNC();
    const int n = w.n;
    if (n < 1) return ekf_fail(w, lane);
    mm(w.T1, w.Phi, S.ekf_P, 5, 5, 5, lane, nl);        // Pp = Phi * P() * transpose(Phi) + Q
    tr(w.PhiT, w.Phi, 5, 5, lane, nl);
    mm(w.T2, w.T1, w.PhiT, 5, 5, 5, lane, nl);
    for (int e = lane; e < 25; e += nl) w.Pp[e] = w.T2[e] + w.Q[e];
    KG_POS_SYNC();
    tr(w.hT, w.h, n, 5, lane, nl);                      // tmp = h * Pp * transpose(h) + R
    mm(w.A, w.h, w.Pp, n, 5, 5, lane, nl);
    mm(w.B, w.A, w.hT, n, 5, n, lane, nl);
    for (int e = lane; e < n * n; e += nl) w.M[e] = w.B[e] + w.W[e];
    KG_POS_SYNC();
    if (lane == 0) lu_factor(w, w.M, n);
    KG_POS_SYNC();
    if (w.det < 1e-30 || w.sing) return ekf_fail(w, lane);      // singular with det not below the gate: the reference's matmult asserts
    lu_inverse(w, n, lane, nl);
    mm(w.B, w.Pp, w.hT, 5, 5, n, lane, nl);             // G = Pp * transpose(h) * cov
    mm(w.G, w.B, w.X, 5, n, n, lane, nl);
    if (lane == 0) {
        for (int r = 0; r < 5; r++) {
            double c = 0;
            for (int j = 0; j < n; j++) c += w.G[r * n + j] * w.dz[j];
            w.dx[r] = c;
        }
        w.ok = !(norm3(w.dx[0], w.dx[1], w.dx[2]) > 1e3);
        if (w.ok) {
            for (int r = 0; r < 5; r++) S.ekf_state[r] = w.xp[r] + w.dx[r];
            S.ekf_state[3] = mod_gpsweek_abs(S.ekf_state[3]);
        }
    }
    KG_POS_SYNC();
    if (!w.ok) return ekf_fail(w, lane);
    mm(w.T1, w.G, w.h, 5, n, 5, lane, nl);              // P = (eye(5) - G * h) * Pp
    for (int e = lane; e < 25; e += nl) w.T2[e] = ((e / 5 == e % 5) ? 1.0 : 0.0) - w.T1[e];
    KG_POS_SYNC();
    mm(S.ekf_P, w.T2, w.Pp, 5, 5, 5, lane, nl);
    if (lane == 0) S.ekf_valid = 1;
    KG_POS_SYNC();
    return true;
}

// ---- PosSolverImpl
KG_POS_FN double dadc_ticks_sec(const uint64_t *t, double f_osc)                        // PosSolver.cpp:169-172
{
    return (t[0] + (t[0] < t[1]) * (1ULL << 48) - t[1]) / f_osc;
}

KG_POS_FN void set_use_kalman(solver &S, int b)         // PosSolver.cpp:32-38
{
    if (!b) {
        S.ekf_running = -1;
        S.state_spp[0] = S.state_spp[1] = 0;
    }
}

KG_POS_FN void solver_init(solver &S)                   // PosSolverImpl's constructor; TNT leaves _state and _cov unset: zero here
{
    unsigned char *p = (unsigned char *) &S;
    for (unsigned i = 0; i < sizeof(solver); i++) p[i] = 0;
    S.osc_corr = -1;
    S.alt = 6371e3;                                     // LonLatAlt's default (PosSolver.h:33)
    S.ekf_running = -1;
}

// solve (PosSolver.cpp:64-144) on the set in w.sv / w.wgt / w.nsv; nsv == 0 returns before anything changes
KG_POS_FN bool solve(ws &w, double uere, double f_osc, int use_kalman, uint64_t adc_ticks, int lane, int nl)
{
    solver &S = w.S;
    const int n = w.nsv;
    if (!n) return false;
    if (lane == 0) {
        double sum = 0;
        for (int i = 0; i < n; i++) sum += w.wgt[i];
        const double scale = sum / (double) n * uere * uere;
        for (int i = 0; i < n; i++) w.wgt[i] /= scale;
        S.ticks_spp[1] = S.ticks_spp[0];
        S.ticks_ekf[0] = S.ticks_spp[0] = adc_ticks;
        make_diag(w.W, w.wgt, n);
    }
    KG_POS_SYNC();
    const bool status = spp_solve(w, lane, nl);
    if (lane == 0) {
        S.state_spp[1] = S.state_spp[0];
        double lambda, phi, altitude;
        xyz2llh(S.spp_state[0], S.spp_state[1], S.spp_state[2], &lambda, &phi, &altitude);
        S.state_spp[0] = (status && altitude > -100 && altitude < 9000);
        S.ct_rx[1] = S.ct_rx[0];
        S.ct_rx[0] = S.spp_state[3];
        if (S.state_spp[0]) {
            S.lambda = lambda; S.phi = phi; S.alt = altitude;
            S.t_rx = S.spp_state[3] / C_LIGHT;
            S.pos[0] = S.spp_state[0]; S.pos[1] = S.spp_state[1]; S.pos[2] = S.spp_state[2];
            S.pos_valid = 1;
        }
        if (S.state_spp[0] && S.state_spp[1]) {
            const double dt_adc_sec = dadc_ticks_sec(S.ticks_spp, f_osc);
            S.osc_corr = mod_gpsweek_rel(S.ct_rx[0] - S.ct_rx[1]) / C_LIGHT / dt_adc_sec;
            if (use_kalman && S.ekf_running == -1) {
                for (int i = 0; i < 25; i++) S.ekf_P[i] = 0.0;
                for (int i = 0; i < 4; i++)
                    for (int j = 0; j < 4; j++) S.ekf_P[i * 5 + j] = S.spp_cov[i * 4 + j];
                S.ekf_P[24] = 1.0;
                for (int i = 0; i < 4; i++) S.ekf_state[i] = S.spp_state[i];
                S.ekf_state[4] = S.osc_corr * C_LIGHT;
                S.ticks_ekf[1] = S.ticks_ekf[0];
                S.ekf_running = 0;
            }
        }
        w.run_ekf = use_kalman && S.ekf_running >= 0;
        w.dt = dadc_ticks_sec(S.ticks_ekf, f_osc);
    }
    KG_POS_SYNC();
    if (w.run_ekf) {
        const bool up = ekf_update(w, w.dt, lane, nl);
        if (lane == 0) {
            if (up) {
                S.ticks_ekf[1] = S.ticks_ekf[0];
                S.ekf_running += (S.ekf_running < 4);
                xyz2llh(S.ekf_state[0], S.ekf_state[1], S.ekf_state[2], &S.lambda, &S.phi, &S.alt);
                S.t_rx = S.ekf_state[3] / C_LIGHT;
                S.osc_corr = S.ekf_state[4] / C_LIGHT;
                S.pos_valid = 1;
                S.pos[0] = S.ekf_state[0]; S.pos[1] = S.ekf_state[1]; S.pos[2] = S.ekf_state[2];
            } else {
                S.ekf_running = -1;
            }
        }
        KG_POS_SYNC();
    }
    return true;
}

// ---- GNSSDataForEpoch::LoadFromReplicas (solve.cpp:319-364) on what kg_eph_sv_dev left: serial.  Row r is channel r; NOT_VALID and
// skipped rows were never in Replicas; `i` counts Replicas, `chans` the rows that enter.  _type[_chans] = Sats[_sat[i]].type reads the
// COMPACTED _sat with i: behind a power-gated row that is _sat[i] == 0 (cleared), Sats[0]'s type.
KG_POS_FN void load_epoch(epoch_in &ep, const snap *snaps, const svrow *rows, int nrow, uint32_t skip, const int32_t *kinds)
{
    for (int k = 0; k < MAXN; k++) {
        ep.sv[0][k] = ep.sv[1][k] = ep.sv[2][k] = ep.sv[3][k] = 0; ep.weight[k] = 0;
        ep.sat[k] = ep.ch[k] = ep.type[k] = ep.week[k] = 0;
    }
    int i = 0, chans = 0;
    for (int r = 0; r < nrow; r++) {
        const int32_t flags = rows[r].flags;
        if ((flags & SV_NOT_VALID) || ((skip >> r) & 1u)) continue;
        if (flags & SV_POWER) { i++; continue; }
        ep.weight[chans] = (double) snaps[r].power;
        ep.sv[3][chans] = rows[r].ct;
        ep.sv[0][chans] = rows[r].x; ep.sv[1][chans] = rows[r].y; ep.sv[2][chans] = rows[r].z;
        ep.sat[chans] = snaps[r].sat;
        ep.ch[chans] = r;
        ep.type[chans] = kinds[ep.sat[i] & (MAX_SATS - 1)];
        ep.week[chans] = rows[r].week;
        chans += 1;
        i++;
    }
    ep.chans = chans; ep.good = i;
}

// the set of solver `which` (0: all, 1: type != E1B, 2: type == E1B; solve.cpp:577-578, :625-637) into the workspace; lane 0
KG_POS_FN void select_set(ws &w, const epoch_in &ep, int which)
{
    int n = 0;
    for (int i = 0; i < ep.chans; i++) {
        if (which == 1 && !(ep.type[i] != KIND_E1B)) continue;
        if (which == 2 && !(ep.type[i] == KIND_E1B)) continue;
        for (int j = 0; j < 4; j++) w.sv[j][n] = ep.sv[j][i];
        w.wgt[n] = ep.weight[i];
        ++n;
    }
    w.nsv = n;
}

KG_POS_FN void report(const solver &S, int called, int nsv, fix *f)
{
    f->x = S.pos[0]; f->y = S.pos[1]; f->z = S.pos[2];
    f->t_rx = S.t_rx; f->osc_corr = S.osc_corr;
    f->lambda = S.lambda; f->phi = S.phi; f->alt = S.alt;
    f->flags = (called ? F_CALLED : 0) | (S.pos_valid ? F_POS_VALID : 0) | (S.state_spp[0] ? F_SPP_VALID : 0) | (S.ekf_running >= 1 ? F_EKF_VALID : 0);
    f->ekf_running = S.ekf_running; f->nsv = nsv; f->pad = 0;
}

// one satellite of IterElevAzim (PositionSolverBase.h:61-70, :108-125) and of the az/el rule (solve.cpp:511-516); m: dENUdXYZ
KG_POS_FN void elev_azim_sat(double ux, double uy, double uz, const double *m, double x, double y, double z, satrec *o)
{
    double d0 = ux - x, d1 = uy - y, d2 = uz - z;
    double cdt = norm3(d0, d1, d2);
    double theta_old = 0;
    for (int i = 0; i < 5; ++i) {
        const double theta = -cdt / C_LIGHT * OMEGA_E;
        rot_diff(theta, x, y, z, ux, uy, uz, &d0, &d1, &d2);
        cdt = norm3(d0, d1, d2);
        if (fabs(theta - theta_old) < 1e-9) break;
        theta_old = theta;
    }
    const double v0 = d0 * -1.0, v1 = d1 * -1.0, v2 = d2 * -1.0;
    double e0 = 0, e1 = 0, e2 = 0;
    e0 += m[0] * v0; e0 += m[1] * v1; e0 += m[2] * v2;
    e1 += m[3] * v0; e1 += m[4] * v1; e1 += m[5] * v2;
    e2 += m[6] * v0; e2 += m[7] * v1; e2 += m[8] * v2;
    const double en = norm3(e0, e1, e2);
    e0 /= en; e1 /= en; e2 /= en;
    const double elev_rad = asin(e2);
    const double azim_rad = atan2(e0, e1);
    const double azim = azim_rad + (azim_rad < 0) * 2 * PI_M;
    o->elev_deg = elev_rad / PI_M * 180;
    o->azim_deg = azim / PI_M * 180;
    const double re = round(o->elev_deg), ra = round(o->azim_deg);
    int el = 0, az = 0;
    if (re == re && ra == ra && fabs(re) < 1e9 && fabs(ra) < 1e9) {     // a NaN converts to INT_MIN on the reference's host: az < 0
        el = (int) re; az = (int) ra;
        if (az < 0 || az >= 360 || el <= 0 || el > 90) el = az = 0;
    }
    o->el = el; o->az = az;
}

// One epoch of SolveTask's loop (solve.cpp:616-641) for solver `which`, whose state is in w.S; ep is formed.  Solver 0 also writes the
// epoch's satellites, chans, grn_yel_red and ch_has_soln.
KG_POS_FN void epoch_step(ws &w, const epoch_in &ep, int which, int use_kalman, int plot_e1b, double uere, double f_osc, uint64_t ticks, epoch_out *out,
                          int lane, int nl)
{
    solver &S = w.S;
    int called = 0;
    if (ep.good != 0) {                                 // `if (good == 0) continue;`
        if (lane == 0) {
            set_use_kalman(S, use_kalman);
            select_set(w, ep, which);
        }
        KG_POS_SYNC();
        if (ep.chans > 0 && (which == 0 || plot_e1b)) called = solve(w, uere, f_osc, use_kalman, ticks, lane, nl);
    }
    if (lane == 0) report(S, called, called ? w.nsv : 0, &out->f[which]);
    if (which != 0) return;
    const bool valid = S.state_spp[0] || S.ekf_running >= 1;
    const bool ekf = S.ekf_running >= 1;
    const double ux = ekf ? S.ekf_state[0] : S.spp_state[0], uy = ekf ? S.ekf_state[1] : S.spp_state[1], uz = ekf ? S.ekf_state[2] : S.spp_state[2];
    if (lane == 0) {
        uint32_t bitmap = 0;
        for (int i = 0; i < ep.chans; i++) bitmap |= 1u << ep.ch[i];
        out->chans = ep.chans;
        out->grn_yel_red = ekf ? 0 : (S.state_spp[0] ? 1 : 2);
        out->ch_has_soln = bitmap; out->pad = 0;
        if (valid) {
            double lambda, phi, alt;
            xyz2llh(ux, uy, uz, &lambda, &phi, &alt);
            dxyz_denu(lambda, phi, w.h3);
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) w.h3T[j * 3 + i] = w.h3[i * 3 + j];
        }
    }
    KG_POS_SYNC();
    for (int i = lane; i < MAXN; i += nl) {
        satrec o;
        o.elev_deg = 0; o.azim_deg = 0; o.sat = o.ch = o.type = o.week = o.el = o.az = 0;
        if (i < ep.chans) {
            o.sat = ep.sat[i]; o.ch = ep.ch[i]; o.type = ep.type[i]; o.week = ep.week[i];
            if (valid) elev_azim_sat(ux, uy, uz, w.h3T, ep.sv[0][i], ep.sv[1][i], ep.sv[2][i], &o);
        }
        out->sat[i] = o;
    }
    KG_POS_SYNC();
}

}  // namespace kg_pos_cf
