// nav_host_driver.cpp -- flydog_sdr_gps_amd/csrc/kg_nav.h compiled by a host compiler and run as the kernels run it, one "lane" at a
// time: the window from the held tail and the new bits, every head offset judged on its own (the Viterbi butterfly per state over a
// metric array, the decision words kept for the chainback), then the walk.  tests/test_nav_cpu.py compares its output with the model
// and the golden records, once as built plainly and once under -fsanitize=address,undefined.
//
// script (stdin): "T <mode>" a fresh channel; "P <bits as 0/1 characters>" a push; "E <Inav flags as 0/1 characters>" a push of epochs
// through the nav-bit machine.  Output per record "F <bit> <err> <consumed> <inverted> <id> <80 hex digits>", per push
// "H <holding> <index of buf[0]> <pushed> <nav_ms> <nav_prev> <nav_glitch> <held bits> <bound on the records>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <iostream>
#include <string>
#include <vector>

#include "../flydog_sdr_gps_amd/csrc/kg_nav.h"

using namespace kg_nav_cf;

struct host_decisions {
    const uint64_t *d;
    uint64_t operator()(uint32_t t) const { return d[t]; }
};

static void decode_half(const uint32_t *w, uint32_t q, uint32_t inv, uint64_t *o0, uint64_t *o1)
{
    uint32_t metric[64], next[64];
    uint64_t dec[120];
    for (int s = 0; s < 64; s++) metric[s] = s ? 63 : 0;
    for (uint32_t t = 0; t < 120; t++) {
        const uint32_t sym0 = e1b_enc(w, q, 2 * t, inv) * 255, sym1 = e1b_enc(w, q, 2 * t + 1, inv) * 255;
        uint64_t word = 0;
        for (uint32_t s = 0; s < 64; s++) {
            uint32_t d;
            next[s] = v27_step(s, metric[s >> 1], metric[(s >> 1) + 32], sym0, sym1, &d);
            word |= (uint64_t) d << s;
        }
        dec[t] = word;
        memcpy(metric, next, sizeof metric);
    }
    v27_chainback(host_decisions{dec}, o0, o1);
}

static void push(chan &c, const std::vector<uint8_t> &bits)
{
    const uint32_t W = (uint32_t) c.holding + (uint32_t) bits.size();
    std::vector<uint32_t> win(W / 32 + 3, 0);
    for (uint32_t i = 0; i < W; i++) {
        const uint32_t b = i < (uint32_t) c.holding ? (c.held[i >> 5] >> (31 - (i & 31))) & 1 : bits[i - c.holding] & 1;
        win[i >> 5] |= b << (31 - (i & 31));
    }
    c.wlen = (int32_t) W; c.nnew = (int32_t) bits.size();
    const int32_t sub = c.mode == MODE_E1B ? E1B_BITS : L1_BITS;
    std::vector<uint64_t> match(W / 64 + 2, 0);
    std::vector<res> rs(W + 1);
    for (int32_t o = 0; o + sub <= (int32_t) W; o++) {
        res r;
        memset(&r, 0, sizeof r);
        if (c.mode == MODE_L1) {
            r.code = (int32_t) l1_judge(win.data(), (uint32_t) o);
        } else {
            const uint32_t pre = e1b_pre(win.data(), (uint32_t) o);
            if (pre) {
                decode_half(win.data(), (uint32_t) o + 10, pre - 1, &r.w[0], &r.w[1]);
                decode_half(win.data(), (uint32_t) o + 10 + E1B_HALF, pre - 1, &r.w[2], &r.w[3]);
                const int32_t err = e1b_page(r.w[0], r.w[1], r.w[2], r.w[3], &r.id);
                r.code = 0x100 | (int32_t) ((pre - 1) << 7) | err;
            }
        }
        if (r.code) { match[o >> 6] |= (uint64_t) 1 << (o & 63); rs[o] = r; }
    }
    const int64_t bound = max_records(c.mode, (int64_t) bits.size());
    std::vector<frame> out((size_t) bound + 1);
    const int32_t n = walk(c, win.data(), match.data(), rs.data(), out.data(), (int32_t) bound + 1);
    for (int32_t k = 0; k < n; k++) {
        const frame &f = out[k];
        printf("F %llu %d %d %d %d ", (unsigned long long) f.bit, f.err, f.consumed, f.inverted, f.id);
        for (int i = 0; i < 40; i++) printf("%02x", f.data[i]);
        printf("\n");
    }
    printf("H %d %llu %llu %u %u %u ", c.holding, (unsigned long long) c.base, (unsigned long long) c.pushed, c.nav_ms, c.nav_prev, c.nav_glitch);
    for (int32_t i = 0; i < c.holding; i++) putchar('0' + ((c.held[i >> 5] >> (31 - (i & 31))) & 1));
    printf(" %lld\n", (long long) bound);
}

int main()
{
    chan c;
    memset(&c, 0, sizeof c);
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::vector<uint8_t> v;
        for (size_t i = 2; i < line.size(); i++)
            if (line[i] == '0' || line[i] == '1') v.push_back((uint8_t) (line[i] - '0'));
        if (line[0] == 'T') {
            memset(&c, 0, sizeof c);
            c.mode = atoi(line.c_str() + 2);
        } else if (line[0] == 'P') {
            push(c, v);
        } else if (line[0] == 'E') {
            std::vector<uint8_t> bits;
            for (uint8_t inav : v)
                if (nav_bit_step(c.mode, &c.nav_ms, &c.nav_prev, &c.nav_glitch, inav)) bits.push_back(inav);
            push(c, bits);
        }
    }
    return 0;
}
