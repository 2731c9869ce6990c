// fix_dropin.cpp -- satellite rows -> position fix through include/kiwigpu.h only (no HIP, no torch): the sequence INTEGRATION.md
// section 6d maps onto the reference's gps/solve.cpp and gps/PosSolver.cpp.
//
//   SolveTask             PosSolver::make(UERE, ADC_CLOCK_TYP) x 3                       -> kg_pos_create
//   SolveTask             admcfg plot_E1B / use_kalman_position_solver, set_use_kalman   -> kg_pos_set_mode
//   LoadFromReplicas      the compaction of the ready channels                           -> kg_pos_solve (inside)
//   SolveTask             posSolvers[0..2]->solve                                        -> kg_pos_solve
//   update_gps_info_after grn_yel_red, ch_has_soln, az/el                                -> the kg_pos_epoch record
//
//   fix_dropin
// Places six satellites around a receiver at 48.2 N 16.3 E 200 m (the rows kg_eph_sv would make, built here from the geometry), solves
// four epochs one second apart and prints the fix.  output per epoch: "fix <flags> ekf <d> nsv <d> lat <f> lon <f> alt <f> t_rx <f>",
// then per satellite of the last epoch "ch <d> sat <d> el <d> az <d>".
#include "kiwigpu.h"

#include <cmath>
#include <cstdio>
#include <cstring>

#define CHECK(call)                                                                      \
    do {                                                                                 \
        int rc_ = (call);                                                                \
        if (rc_ < 0) { fprintf(stderr, "%s -> %s\n", #call, kg_last_error()); return 1; } \
    } while (0)

static const double PI = 3.14159265358979323846, C = 2.99792458e8, OMEGA_E = 7.2921151467e-5, A = 6378137.0, B = 6356752.31424518;

int main()
{
    kg_ctx *ctx = nullptr;
    kg_pos *pos = nullptr;
    int32_t kinds[64];
    for (int k = 0; k < 64; k++) kinds[k] = k < 32 ? KG_EPH_NAVSTAR : (k < 36 ? KG_EPH_CA : KG_EPH_E1B);     // the order of the reference's Sats[]
    CHECK(kg_ctx_create(0, nullptr, &ctx));
    CHECK(kg_pos_create(ctx, kinds, 6.0, 124.9999e6, &pos));
    CHECK(kg_pos_set_mode(pos, 1, 1));

    const double lat = 48.2 * PI / 180, lon = 16.3 * PI / 180, alt = 200.0;
    const double e2 = 1.0 - (B * B) / (A * A), nu = A / sqrt(1.0 - e2 * sin(lat) * sin(lat));
    const double p[3] = {(nu + alt) * cos(lat) * cos(lon), (nu + alt) * cos(lat) * sin(lon), ((1 - e2) * nu + alt) * sin(lat)};
    const double east[3] = {-sin(lon), cos(lon), 0}, north[3] = {-sin(lat) * cos(lon), -sin(lat) * sin(lon), cos(lat)},
                 up[3] = {cos(lat) * cos(lon), cos(lat) * sin(lon), sin(lat)};
    const int NSAT = 6, NEPOCH = 4;
    const double az[NSAT] = {20, 100, 190, 250, 310, 355}, el[NSAT] = {70, 25, 40, 15, 55, 30};
    const int sat[NSAT] = {1, 7, 12, 20, 40, 45};           // four Navstar, two Galileo
    kg_eph_snap snaps[NEPOCH * NSAT];
    kg_eph_pos sv[NEPOCH * NSAT];
    uint64_t ticks[NEPOCH];
    memset(snaps, 0, sizeof snaps); memset(sv, 0, sizeof sv);
    for (int e = 0; e < NEPOCH; e++) {
        const double t_rx = 200000.0 + e;                   // the receiver's clock at reception, seconds of week
        ticks[e] = 1000 + (uint64_t) e * 124999900ull;
        for (int i = 0; i < NSAT; i++) {
            const double a = az[i] * PI / 180, h = el[i] * PI / 180, u[3] = {sin(a) * cos(h), cos(a) * cos(h), sin(h)};
            double dir[3], b = 0, pp = 0;
            for (int k = 0; k < 3; k++) { dir[k] = east[k] * u[0] + north[k] * u[1] + up[k] * u[2]; b += p[k] * dir[k]; pp += p[k] * p[k]; }
            const double d = -b + sqrt(b * b - (pp - 26.56e6 * 26.56e6));              // the range to a satellite 26 560 km from the centre
            const double s[3] = {p[0] + d * dir[0], p[1] + d * dir[1], p[2] + d * dir[2]}, th = d / C * OMEGA_E;
            kg_eph_pos &r = sv[e * NSAT + i];
            r.x = cos(th) * s[0] - sin(th) * s[1]; r.y = sin(th) * s[0] + cos(th) * s[1]; r.z = s[2];         // in the frame of its transmit time
            r.ct = C * t_rx - d; r.week = 2200; r.flags = 0;
            snaps[e * NSAT + i].sat = sat[i]; snaps[e * NSAT + i].power = 1e6f;
        }
    }
    kg_pos_epoch out[NEPOCH];
    CHECK(kg_pos_solve(pos, snaps, sv, NSAT, NEPOCH, ticks, nullptr, out));
    for (int e = 0; e < NEPOCH; e++) {
        const kg_pos_fix &f = out[e].fix[0];
        printf("fix %d ekf %d nsv %d lat %.7f lon %.7f alt %.3f t_rx %.9f\n", f.flags, f.ekf_running, f.nsv, f.phi * 180 / PI, f.lambda * 180 / PI, f.alt, f.t_rx);
    }
    for (int i = 0; i < out[NEPOCH - 1].chans; i++) {
        const kg_pos_sat &s = out[NEPOCH - 1].sat[i];
        printf("ch %d sat %d el %d az %d\n", s.ch, s.sat, s.el, s.az);
    }
    const kg_pos_fix &last = out[NEPOCH - 1].fix[0];
    if (!(last.flags & KG_POS_EKF_VALID) || fabs(last.phi - lat) > 1e-7 || fabs(last.lambda - lon) > 1e-7 || fabs(last.alt - alt) > 1.0 ||
        out[NEPOCH - 1].grn_yel_red != 0 || out[NEPOCH - 1].fix[1].nsv != 4 || out[NEPOCH - 1].fix[2].nsv != 2) {
        fprintf(stderr, "the fix did not come out where the receiver was placed\n");
        return 1;
    }
    kg_pos_state st;
    CHECK(kg_pos_get_state(pos, 0, &st));
    printf("solver 0: ekf_running %d, P(0,0) %.3e m^2\n", st.ekf_running, st.ekf_P[0]);
    kg_pos_destroy(pos);
    kg_ctx_destroy(ctx);
    return 0;
}
