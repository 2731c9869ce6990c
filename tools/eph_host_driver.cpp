// eph_host_driver.cpp -- csrc/kg_eph.h compiled for the host: the same statements the kernels run, as a stand-alone program
// (tests/test_eph_cpu.py builds it plainly and under the address / undefined-behaviour sanitizers).
//
// script (stdin):
//   B <ch> <sat> <kind>                        kg_eph_set_sat
//   F <ch> <err> <bit> <consumed> <80 hex>     one kg_nav_frame of the channel: the field step, then the walk step
//   V <sat> <bits> <bits_tow> <ms> <chips> <cg_phase> <power as %a>
//   R <replica word>
// output:
//   per frame     "E <week_gst> <toes> <toc_gst> <delta_tLS> <delta_tLSF> <tLS_valid> <64 hex: the note> <624 hex: the satellite's kg_ephem>"
//   per snapshot  "V <flags> <clock %a> <ct> <t_k> <x> <y> <z> <week>" (clock: GetClock alone; 0 when the snapshot was refused before it)
//   per word      "R <chips> <cg_phase>"
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <iostream>
#include <string>

#include "../flydog_sdr_gps_amd/csrc/kg_eph.h"

using namespace kg_eph_cf;

static ephem slots[MAX_SATS];
static chanst chans[12];
static utc leap;

static void hex(const void *p, size_t n)
{
    const uint8_t *b = (const uint8_t *) p;
    for (size_t i = 0; i < n; i++) printf("%02x", b[i]);
}

int main()
{
    memset(slots, 0, sizeof slots); memset(chans, 0, sizeof chans); memset(&leap, 0, sizeof leap);
    for (int ch = 0; ch < 12; ch++) chans[ch].sat = -1;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        const char *p = line.c_str() + 2;
        if (line[0] == 'B') {
            int ch, sat, kind;
            if (sscanf(p, "%d %d %d", &ch, &sat, &kind) != 3 || ch < 0 || ch >= 12 || sat < -1 || sat >= MAX_SATS) return 2;
            chans[ch].sat = sat; chans[ch].kind = kind;
            if (sat >= 0) { slots[sat].kind = (uint32_t) kind; slots[sat].valid = valid(slots[sat]); }
        } else if (line[0] == 'F') {
            int ch, err, consumed, n = 0;
            unsigned long long bit;
            if (sscanf(p, "%d %d %llu %d %n", &ch, &err, &bit, &consumed, &n) != 4 || ch < 0 || ch >= 12) return 2;
            uint8_t data[40];
            if (strlen(p + n) < 80) return 2;
            for (int i = 0; i < 40; i++) { unsigned v; if (sscanf(p + n + 2 * i, "%2x", &v) != 1) return 2; data[i] = (uint8_t) v; }
            upd o;
            fields(chans[ch].kind, err, data, o);
            note nt;
            int32_t has = 0;
            utc l = leap;
            step(slots, chans[ch], o, (uint64_t) bit + (uint64_t) (int64_t) consumed, &nt, &l, &has);
            if (has) leap = l;
            printf("E %u %u %u %d %d %d ", chans[ch].week_gst, chans[ch].toes, chans[ch].toc_gst, leap.delta_tLS, leap.delta_tLSF, leap.tLS_valid);
            hex(&nt, sizeof nt);
            printf(" ");
            if (chans[ch].sat >= 0) hex(&slots[chans[ch].sat], sizeof(ephem));
            printf("\n");
        } else if (line[0] == 'V') {
            snap s;
            double power;
            if (sscanf(p, "%d %d %d %d %d %d %la", &s.sat, &s.bits, &s.bits_tow, &s.ms, &s.chips, &s.cg_phase, &power) != 7) return 2;
            s.power = (float) power;
            sv o;
            memset(&o, 0, sizeof o);
            sv_one(slots, s, &o);
            double clock = 0;
            if (!(o.flags & (SV_NOT_VALID | SV_POWER))) {
                int32_t f = 0;
                clock = get_clock(slots[s.sat], s, &f);
            }
            printf("V %d %a %a %a %a %a %a %d\n", o.flags, clock, o.ct, o.t_k, o.x, o.y, o.z, o.week);
        } else if (line[0] == 'R') {
            unsigned word;
            if (sscanf(p, "%u", &word) != 1) return 2;
            int32_t chips, cg;
            replica_split(word, &chips, &cg);
            printf("R %d %d\n", chips, cg);
        }
    }
    return 0;
}
