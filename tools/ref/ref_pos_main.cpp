// ref_pos_main.cpp -- the harness tools/make_ref_pos_golden.py compiles around the reference's position solver at build time (nothing of
// the reference is committed): gps/PosSolver.cpp with its headers and pkgs/TNT_JAMA, compiled from the reference tree as they are (this
// file includes PosSolver.cpp with `private` and `protected` read as `public`, so that the solvers' members can be printed), and text CUT
// from gps/solve.cpp and gps/gps.h:
//
//     gps/gps.h      UMS (:289-296)
//     gps/solve.cpp  class GNSSDataForEpoch (:251-389); SolveTask's three solvers and predicates (:571-578) and its per-epoch statements,
//                    `if (good == 0) continue;` to the last solve (:616-639); update_gps_info_after's grn_yel_red (:497-498) and az/el
//                    rule up to its rejection (:501-516)
//   restated here and pinned by text in the generator: UERE (solve.cpp:38), ADC_CLOCK_TYP (init/clk.h:30) -- variables here, set by the
//     script to the pinned values --, the sat_e order (gps.h:98), C (gps.h:92), the members of SNAPSHOT and EPHEM the cut text names, the
//     kiwi_next_task of solve.cpp:557-565.
//
// The replicas are stand-ins: GetClock returns ct / C, GetClockCorrection 0, GetXYZ the row's x, y, z -- the rows of kg_eph_sv_dev are the
// input here, kg_eph's own pin made them.  The generator gives only ct with C * (ct / C) == ct (checked here).  TNT leaves a fresh
// solver's _state and _cov unset; the harness zeroes them, as kg_pos starts.
//
// script (stdin) and output: those of tools/pos_host_driver.cpp, with `type` as sat_e (Navstar 0, QZSS 2, E1B 3) in K and S.
#include <assert.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <array>
#include <cmath>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#define private public
#define protected public
#include "PosSolver.cpp"
#undef private
#undef protected

typedef unsigned int u4_t;
typedef unsigned long long u64_t;
#define MAX_SATS 64
#define GPS_MAX_CHANS 12
#define GPS_N_AGE 9
#define NextTask(s) ((void) 0)
#define CFG_REQUIRED 0
static const double C = 2.99792458e8;
static double UERE, ADC_CLOCK_TYP;

#include POS_CUT_UMS

typedef enum { Navstar, SBAS, QZSS, E1B } sat_e;
static struct { int prn; sat_e type; } Sats[MAX_SATS];
static struct {
    struct { bool too_old; char age[GPS_N_AGE]; } ch[GPS_MAX_CHANS];
    int last_samp;
    int el[1][MAX_SATS];
} gps;

struct EPHEM_STANDIN {
    double x, y, z;
    int week;
    double GetClockCorrection(double) const { return 0; }
    double TimeOfEphemerisAge(double) const { return 0; }
    void GetXYZ(double *px, double *py, double *pz, double) const { *px = x; *py = y; *pz = z; }
};
struct SNAPSHOT {
    EPHEM_STANDIN eph;
    float power;
    int ch, sat;
    double t;
    double GetClock() const { return t; }
};
static SNAPSHOT Replicas[GPS_MAX_CHANS];
static int gps_chans = GPS_MAX_CHANS;

#include POS_CUT_EPOCH

class kiwi_next_task : public kiwi_yield {
public:
    kiwi_next_task() {}
    virtual ~kiwi_next_task() {}
    virtual void yield() const {}
};

static bool cfg_plot_E1B = false, cfg_use_kalman = true;
static bool admcfg_bool(const char *, void *, int) { return cfg_plot_E1B; }
static bool admcfg_default_bool(const char *, bool, void *) { return cfg_use_kalman; }

static int rec_gyr, rec_el[GPS_MAX_CHANS], rec_az[GPS_MAX_CHANS];
static u4_t rec_soln;
#define STAT_SOLN 0
#define GPSstat(st, a, b, c) (rec_gyr = (b), rec_soln = (c))

static void after(const GNSSDataForEpoch &gnssDataForEpoch, std::array<PosSolver::sptr, 3> &pos_solvers)
{
    memset(rec_el, 0, sizeof rec_el); memset(rec_az, 0, sizeof rec_az);
#include POS_CUT_GYR
#include POS_CUT_AZEL
            rec_el[i] = el; rec_az[i] = az;
        }
    }
}

static void zero(PosSolver::sptr &p)
{
    PosSolverImpl *s = static_cast<PosSolverImpl *>(p.get());
    s->_spp._state = 0.0; s->_spp._cov = 0.0; s->_ekf._state = 0.0; s->_ekf._cov = 0.0;
}

static void put(const double *v, int n)
{
    for (int i = 0; i < n; i++) printf(" %a", v[i]);
}

int main()
{
    std::string line;
    GNSSDataForEpoch gnssDataForEpoch(gps_chans);
    auto yield = std::make_shared<kiwi_next_task>();
    while (std::getline(std::cin, line)) {              // K and C come first
        if (line[0] == 'K') {
            const char *p = line.c_str() + 1;
            for (int k = 0; k < MAX_SATS; k++) {
                int n = 0, t;
                if (sscanf(p, "%d%n", &t, &n) != 1) return 2;
                Sats[k].type = (sat_e) t; Sats[k].prn = k + 1;
                p += n;
            }
        } else if (line[0] == 'C') {
            if (sscanf(line.c_str() + 1, "%la %la", &UERE, &ADC_CLOCK_TYP) != 2) return 2;
            break;
        } else
            return 2;
    }
#include POS_CUT_SOLVERS
    for (auto &p : posSolvers) zero(p);
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        const char *p = line.c_str() + 1;
        if (line[0] == 'M') {
            int a, b;
            if (sscanf(p, "%d %d", &a, &b) != 2) return 2;
            cfg_use_kalman = a != 0; cfg_plot_E1B = b != 0;
            continue;
        }
        if (line[0] == 'X') {
            for (auto &q : posSolvers) { q = PosSolver::make(UERE, ADC_CLOCK_TYP, yield); zero(q); }
            continue;
        }
        if (line[0] != 'E') return 2;
        int nrow, good = 0;
        unsigned long long ticks;
        unsigned skip;
        if (sscanf(p, "%d %llu %u", &nrow, &ticks, &skip) != 3 || nrow < 1 || nrow > GPS_MAX_CHANS) return 2;
        for (int r = 0; r < nrow; r++) {
            int sat, flags, week;
            double power, x, y, z, ct;
            if (!std::getline(std::cin, line) || line[0] != 'R') return 2;
            if (sscanf(line.c_str() + 1, "%d %d %d %la %la %la %la %la", &sat, &flags, &week, &power, &x, &y, &z, &ct) != 8) return 2;
            if ((flags & 1) || ((skip >> r) & 1)) continue;             // never in Replicas
            const float pw = (float) power;
            if (((flags & 2) != 0) != ((double) pw < 1e5 || (double) pw > 5e6)) return 3;       // the flag is what the reference's gate does
            SNAPSHOT &s = Replicas[good++];
            s.power = pw; s.ch = r; s.sat = sat; s.t = ct / C;
            s.eph.x = x; s.eph.y = y; s.eph.z = z; s.eph.week = week;
            if (!(flags & 2) && ct == ct && C * s.t != ct) return 4;
        }
        bool plot = false;
        for (int once = 0; once < 1; once++) {
#include POS_CUT_SOLVE
            plot = plot_E1B;
        }
        if (good == 0) {                                // SolveTask's `continue`: nothing ran; the record reports what is held
            gnssDataForEpoch.LoadFromReplicas(0, Replicas, ticks);
            plot = false;
        }
        after(gnssDataForEpoch, posSolvers);
        const int chans = gnssDataForEpoch.chans();
        int nsv[3] = { chans, 0, 0 };
        for (int i = 0; i < chans; i++) { nsv[1] += gnssDataForEpoch.type(i) != E1B; nsv[2] += gnssDataForEpoch.type(i) == E1B; }
        if (!plot) nsv[1] = nsv[2] = 0;
        for (int k = 0; k < 3; k++) {
            PosSolverImpl *s = static_cast<PosSolverImpl *>(posSolvers[k].get());
            const int flags = (nsv[k] > 0 ? 1 : 0) | (s->pos_valid() ? 2 : 0) | (s->spp_valid() ? 4 : 0) | (s->ekf_valid() ? 8 : 0);
            printf("F %d %d %d %d %a %a %a %a %a %a %a %a\n", k, flags, s->_ekf_running, nsv[k], s->pos(0), s->pos(1), s->pos(2), s->t_rx(), s->osc_corr(),
                   s->llh().lambda(), s->llh().phi(), s->llh().alt());
        }
        const auto ea = posSolvers[0]->elev_azim(gnssDataForEpoch.sv());
        for (int i = 0; i < chans; i++)
            printf("S %d %d %d %d %d %d %d %a %a\n", i, gnssDataForEpoch.sat(i), gnssDataForEpoch.ch(i), gnssDataForEpoch.type(i), gnssDataForEpoch.week(i),
                   rec_el[i], rec_az[i], ea.empty() ? 0.0 : ea[i].elev_deg, ea.empty() ? 0.0 : ea[i].azim_deg);
        printf("G %d %d %u\n", chans, rec_gyr, rec_soln);
        for (int k = 0; k < 3; k++) {
            PosSolverImpl *s = static_cast<PosSolverImpl *>(posSolvers[k].get());
            printf("T %d %d %d %d %d %llu %llu %llu %llu", k, (int) s->_pos_valid, (int) s->_state_spp[0], (int) s->_state_spp[1], (int) s->_ekf._valid,
                   (unsigned long long) s->_ticks_spp[0], (unsigned long long) s->_ticks_spp[1], (unsigned long long) s->_ticks_ekf[0],
                   (unsigned long long) s->_ticks_ekf[1]);
            put(&s->_ct_rx[0], 2);
            put(&s->_spp._state[0], 4);
            for (int i = 0; i < 4; i++) put(s->_spp._cov[i], 4);
            put(&s->_ekf._state[0], 5);
            for (int i = 0; i < 5; i++) put(s->_ekf._cov[i], 5);
            printf("\n");
        }
    }
    return 0;
}
