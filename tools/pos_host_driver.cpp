// pos_host_driver.cpp -- csrc/kg_pos.h compiled for the host: the same statements the kernel runs, as a stand-alone program
// (tests/test_pos_cpu.py builds it plainly and under the address / undefined-behaviour sanitizers).  One lane: (lane, nl) = (0, 1).
//
// script (stdin; doubles as %a):
//   K <64 kinds>                               the kinds table (KG_EPH_*); before C
//   C <uere> <f_osc>                           kg_pos_create: three fresh solvers, use_kalman 1, plot_e1b 0
//   M <use_kalman> <plot_e1b>                  kg_pos_set_mode
//   X                                          kg_pos_reset
//   E <nrow> <ticks> <skip>                    one epoch; its nrow rows follow
//   R <sat> <flags> <week> <power> <x> <y> <z> <ct>
// output per epoch (the format of tools/ref/ref_pos_main.cpp):
//   F <solver> <flags> <ekf_running> <nsv> <x> <y> <z> <t_rx> <osc_corr> <lambda> <phi> <alt>          three
//   S <i> <sat> <ch> <type> <week> <el> <az> <elev_deg> <azim_deg>                                       chans
//   G <chans> <grn_yel_red> <ch_has_soln>
//   T <solver> <pos_valid> <state_spp 0 1> <ekf_valid> <ticks_spp 0 1> <ticks_ekf 0 1> <ct_rx 0 1> <spp_state 4> <spp_cov 16> <ekf_state 5> <ekf_P 25>   three
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <iostream>
#include <string>

#include "../flydog_sdr_gps_amd/csrc/kg_pos.h"

using namespace kg_pos_cf;

static ws work[3];
static epoch_in ep;
static epoch_out out;
static int32_t kinds[MAX_SATS];
static snap snaps[MAXN];
static svrow rows[MAXN];

static void put(const double *v, int n)
{
    for (int i = 0; i < n; i++) printf(" %a", v[i]);
}

int main()
{
    memset(work, 0, sizeof work); memset(kinds, 0, sizeof kinds);
    double uere = 0, f_osc = 0;
    int use_kalman = 1, plot_e1b = 0, created = 0;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        const char *p = line.c_str() + 1;
        if (line[0] == 'K') {
            for (int k = 0; k < MAX_SATS; k++) {
                int n = 0;
                if (sscanf(p, "%d%n", &kinds[k], &n) != 1 || kinds[k] < 0 || kinds[k] > 2) return 2;
                p += n;
            }
        } else if (line[0] == 'C') {
            if (sscanf(p, "%la %la", &uere, &f_osc) != 2) return 2;
            for (int s = 0; s < 3; s++) solver_init(work[s].S);
            use_kalman = 1; plot_e1b = 0; created = 1;
        } else if (line[0] == 'M') {
            if (sscanf(p, "%d %d", &use_kalman, &plot_e1b) != 2) return 2;
        } else if (line[0] == 'X') {
            for (int s = 0; s < 3; s++) solver_init(work[s].S);
        } else if (line[0] == 'E') {
            int nrow;
            unsigned long long ticks;
            unsigned skip;
            if (!created || sscanf(p, "%d %llu %u", &nrow, &ticks, &skip) != 3 || nrow < 1 || nrow > MAXN) return 2;
            for (int r = 0; r < nrow; r++) {
                double power;
                if (!std::getline(std::cin, line) || line[0] != 'R') return 2;
                memset(&snaps[r], 0, sizeof snaps[r]); memset(&rows[r], 0, sizeof rows[r]);
                if (sscanf(line.c_str() + 1, "%d %d %d %la %la %la %la %la", &snaps[r].sat, &rows[r].flags, &rows[r].week, &power, &rows[r].x, &rows[r].y,
                           &rows[r].z, &rows[r].ct) != 8)
                    return 2;
                snaps[r].power = (float) power;
            }
            load_epoch(ep, snaps, rows, nrow, skip, kinds);
            memset(&out, 0, sizeof out);
            for (int s = 0; s < 3; s++) epoch_step(work[s], ep, s, use_kalman, plot_e1b, uere, f_osc, (uint64_t) ticks, &out, 0, 1);
            for (int s = 0; s < 3; s++) {
                const fix &f = out.f[s];
                printf("F %d %d %d %d", s, f.flags, f.ekf_running, f.nsv);
                put(&f.x, 8);
                printf("\n");
            }
            for (int i = 0; i < out.chans; i++) {
                const satrec &o = out.sat[i];
                printf("S %d %d %d %d %d %d %d %a %a\n", i, o.sat, o.ch, o.type, o.week, o.el, o.az, o.elev_deg, o.azim_deg);
            }
            printf("G %d %d %u\n", out.chans, out.grn_yel_red, out.ch_has_soln);
            for (int s = 0; s < 3; s++) {
                const solver &S = work[s].S;
                printf("T %d %d %d %d %d %llu %llu %llu %llu", s, S.pos_valid, S.state_spp[0], S.state_spp[1], S.ekf_valid, (unsigned long long) S.ticks_spp[0],
                       (unsigned long long) S.ticks_spp[1], (unsigned long long) S.ticks_ekf[0], (unsigned long long) S.ticks_ekf[1]);
                put(S.ct_rx, 2); put(S.spp_state, 4); put(S.spp_cov, 16); put(S.ekf_state, 5); put(S.ekf_P, 25);
                printf("\n");
            }
        } else
            return 2;
    }
    return 0;
}
