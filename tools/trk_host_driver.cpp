// trk_host_driver.cpp -- flydog_sdr_gps_amd/csrc/kg_trk.h, the closed form the tracking kernel runs, compiled for the host as ONE lane
// and driven by the script format of tools/trk_model.cpp (same arguments, same output), so that tests/test_trk_cpu.py can hold it
// equal to the literal model without a GPU.  The command layer below restates kg_trk.hip's state changes and its three KG_ERR_STATE
// refusals (a command that would make a paused channel hold ms0 set: kg_trk.h): such a line changes nothing and is answered with
// "! <number of the line after N, from 0>", so that the caller can take it out of the model's script.  Exit status 7: a channel's code
// loop left the accepted range.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../flydog_sdr_gps_amd/csrc/kg_trk.h"

using namespace kg_trk_cf;

struct one_lane { seg_sums operator()(seg_sums v) const { return v; } };

static std::vector<uint8_t> slurp(const char *path)
{
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: trk_host_driver BITS CODES < script\n"); return 2; }
    const std::vector<uint8_t> bits = slurp(argv[1]), codes = slurp(argv[2]);
    std::vector<chan> h;
    std::vector<chan_tab> tab, e1b;
    int nchan = 0;
    uint32_t cg_cnt = 0, mask = 0;
    uint64_t clock = 0;
    char line[256];
    int step = -2;                                                      // the N line is -1
    while (fgets(line, sizeof line, stdin)) {
        step++;
        char op = 0;
        long long a = 0, b = 0, c = 0;
        if (sscanf(line, " %c %lld %lld %lld", &op, &a, &b, &c) < 1) continue;
        if (op == 'T') {                                                  // close_loop alone
            unsigned long long f = 0; long long e = 0; int ki = 0, kpm = 0;
            sscanf(line, " %c %llu %lld %d %d", &op, &f, &e, &ki, &kpm);
            uint64_t freq = f;
            const uint16_t gain[2] = {(uint16_t) ki, (uint16_t) kpm};
            const uint32_t nco = close_loop(&freq, gain, (uint64_t) e);
            printf("T %llu %u\n", (unsigned long long) freq, nco);
            continue;
        }
        if (op == 'N') {
            nchan = (int) a;
            chan z;
            memset(&z, 0, sizeof z);
            z.cg_en = 1; z.loop_on = 1; z.ms1_due = z.lo_due = z.cg_due = -1; z.lo_delay = (uint32_t) b; z.cg_delay = (uint32_t) c;
            h.assign(nchan, z);
            chan_tab zt;
            memset(&zt, 0, sizeof zt);
            tab.assign(nchan, zt); e1b.assign(nchan, zt);
            continue;
        }
        const bool bank = op == 'M' || op == 'R' || op == 'X' || op == 'D';
        if (!bank && (a < 0 || a >= nchan)) { fprintf(stderr, "bad channel: %s", line); return 2; }
        chan *d = bank ? nullptr : &h[a];
        switch (op) {
        case 'S': d->sat = (uint32_t) b; d->fw.e1b_mode = (uint16_t) (b & E1B_MODE); d->have_sat = 1; d->seeded = 0; break;
        case 'C':
            if ((size_t) (b + 1) * E1B_CODELEN > codes.size()) { fprintf(stderr, "no code block %lld\n", b); return 2; }
            memset(&e1b[a], 0, sizeof(chan_tab));
            for (int i = 0; i < E1B_CODELEN; i++) e1b[a].w[i >> 5] |= (uint32_t) codes[b * E1B_CODELEN + i] << (i & 31);
            d->have_code = 1;
            if (d->sat & E1B_MODE) tab[a] = e1b[a];
            break;
        case 'L': d->fw.lo_freq = (uint64_t) (uint32_t) b << 32; d->lo_rate = (uint32_t) b; break;
        case 'G':
            if (rate_would_hold_ms0(*d, (uint32_t) b)) { printf("! %d\n", step); break; }
            d->fw.cg_freq = (uint64_t) (uint32_t) b << 32; d->cg_rate = (uint32_t) b; d->fault = 0; break;
        case 'l': d->fw.lo_gain[0] = (uint16_t) b; d->fw.lo_gain[1] = (uint16_t) c; break;
        case 'g': d->fw.cg_gain[0] = (uint16_t) b; d->fw.cg_gain[1] = (uint16_t) c; break;
        case 'P': d->fw.lo_polarity = (uint16_t) b; break;
        case 'M': mask = (uint32_t) a; break;
        case 'R': {
            bool refuse = false;
            for (int ch = 0; ch < nchan; ch++) refuse = refuse || (!((mask >> ch) & 1) && reset_would_hold_ms0(h[ch]));
            if (refuse) { printf("! %d\n", step); break; }
            for (int ch = 0; ch < nchan; ch++) {
                if ((mask >> ch) & 1) continue;
                h[ch].cg_phase = 0; h[ch].nchip = 0;
                if (h[ch].have_sat) {
                    if (h[ch].sat & E1B_MODE) tab[ch] = e1b[ch]; else ca_table(h[ch].sat, &tab[ch]);
                    h[ch].seeded = 1;
                }
            }
            break;
        }
        case 'Q': {
            chan_tab t;
            ca_table(d->sat, &t);
            printf("Q %lld ", a);
            for (int k = 0; k < L1_CODELEN; k++) printf("%u", tab_bit(t.w, k));
            printf("\n");
            break;
        }
        case 'U':
            if (pause_would_hold_ms0(*d)) { printf("! %d\n", step); break; }
            d->cg_en = 0; cg_cnt = (uint32_t) b & 0xFFFF; break;
        case 'O': d->loop_on = b != 0; break;
        case 'X': {
            const uint64_t bit0 = clock & 7, nbytes = (bit0 + (uint64_t) a + 7) / 8;
            if ((clock >> 3) + nbytes > bits.size()) { fprintf(stderr, "stream too short\n"); return 2; }
            const int cap = (int) (a / 8184 + 2);
            std::vector<epoch> out(cap);
            for (int ch = 0; ch < nchan; ch++) {
                if (!h[ch].seeded || holds_ms0(h[ch])) { fprintf(stderr, "channel %d cannot run\n", ch); return 6; }
                int n = 0;
                run(h[ch], tab[ch].w, bits.data() + (clock >> 3), nbytes, bit0, (uint64_t) a, clock, cg_cnt, out.data(), cap, &n, 0u, 1u, one_lane());
                if (h[ch].fault) { fprintf(stderr, "channel %d: code rate left the accepted range\n", ch); return 7; }
                for (int i = 0; i < n; i++) {
                    const epoch &r = out[i];
                    printf("E %d %llu %d %d %d %d %d %d %u %u %u\n", ch, (unsigned long long) r.clock, r.ip, r.qp, r.ie, r.qe, r.il, r.ql, r.lo_rate,
                           r.cg_rate, r.flags);
                }
            }
            clock += (uint64_t) a;
            cg_cnt = (uint32_t) ((cg_cnt - (uint64_t) a) & 0xFFFF);
            break;
        }
        case 'D':
            for (int ch = 0; ch < nchan; ch++) {
                printf("C %d ", ch);
                const uint8_t *m = (const uint8_t *) &h[ch].fw;
                for (int i = 0; i < CHAN_BYTES; i++) printf("%02x", m[i]);
                printf("\n");
            }
            printf("K %llu", (unsigned long long) clock);
            for (int ch = 0; ch < nchan; ch++) printf(" %u", replica(h[ch]));
            printf("\n");
            break;
        default: fprintf(stderr, "bad line: %s", line); return 2;
        }
    }
    return 0;
}
