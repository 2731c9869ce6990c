// Host driver of csrc/kg_iqd.h (tests/iqd_common.py compiles it with g++ -O2 -ffp-contract=off, the reference's flags): the IQ display
// extension's commands, PLLs, means, byte mapping, rings and rows, with the script language and the output layout of
// tools/ref/ref_iqd_main.cpp.
//   iqd_host_driver script.txt pool.bin out.bin
// Exit status 10 + the refusal's number (11: a negative exponent, 12: points outside 1 .. 16384, 13: the sample rate, 14: a block
// before `N` or before a rate) when kg_iqd.h refuses; out.bin then holds what came before.
#include "../flydog_sdr_gps_amd/csrc/kg_iqd.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace kg_iqd_cf;

static std::vector<unsigned char> slurp(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    std::vector<unsigned char> v;
    unsigned char buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

static std::vector<unsigned char> sent_rows;
static int nrows;
static void emit(void *, int, int cmd, const unsigned char *bytes, int nbytes)
{
    const int32_t h[2] = {cmd, nbytes};
    sent_rows.insert(sent_rows.end(), (const unsigned char *) h, (const unsigned char *) h + 8);
    sent_rows.insert(sent_rows.end(), bytes, bytes + nbytes);
    nrows++;
}

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s script.txt pool.bin out.bin\n", argv[0]); return 2; }
    static full_t q;                                                    // all zero: not initialised
    FILE *sf = fopen(argv[1], "r"), *of = fopen(argv[3], "wb");
    if (!sf || !of) return 2;
    const std::vector<unsigned char> pool = slurp(argv[2]);
    const size_t npool = pool.size() / 8;
    char line[256];
    int refused = 0;
    while (!refused && fgets(line, sizeof line, sf)) {
        line[strcspn(line, "\n")] = 0;
        const char op = line[0];
        int a = 0, b = 0;
        if (op == 'N') {
            memset(&q, 0, sizeof q);
            fresh(q.s);
        } else if (op == 0 || op == '#') {
        } else if (!q.s.inited) {
            refused = 14;
        } else if (op == 'R') {
            double rate;
            if (sscanf(line + 1, "%d %lf", &a, &rate) != 2) return 3;
            if (cmd_run(q.s, a, rate)) refused = 13;
        } else if (op == 'G') {
            if (sscanf(line + 1, "%d", &a) != 1) return 3;
            cmd_gain(q.s, a);
        } else if (op == 'P') {
            if (sscanf(line + 1, "%d", &a) != 1) return 3;
            if (cmd_points(q.s, a)) refused = 12;
        } else if (op == 'M') {
            if (sscanf(line + 1, "%d %d", &a, &b) != 2) return 3;
            if (cmd_pll_mode(q.s, a, b)) refused = 11;
        } else if (op == 'W') {
            float bw;
            if (sscanf(line + 1, "%f", &bw) != 1) return 3;
            cmd_pll_bandwidth(q.s, bw);
        } else if (op == 'D') {
            if (sscanf(line + 1, "%d", &a) != 1) return 3;
            cmd_draw(q.s, a);
        } else if (op == 'Y') {
            if (sscanf(line + 1, "%d", &a) != 1) return 3;
            cmd_display_mode(q.s, a);
        } else if (op == 'C') {
            cmd_clear(q.s);
        } else if (op == 'B') {
            int inst, ns;
            unsigned long off;
            if (sscanf(line + 1, "%d %d %lu", &inst, &ns, &off) != 3 || ns < 1 || ns > MAX_NS || off + ns > npool || inst < 0 || inst > 1) return 3;
            if (!q.s.rate_set) { refused = 14; break; }
            sent_rows.clear();
            nrows = 0;
            int sent = 0;
            status_t st;
            memset(&st, 0, sizeof st);
            if (q.s.run) display_data(q, inst, ns, (const float *) (pool.data() + 8 * off), emit, nullptr, &sent, &st);
            fwrite(&nrows, 4, 1, of);
            if (!sent_rows.empty()) fwrite(sent_rows.data(), 1, sent_rows.size(), of);
            fwrite(&sent, 4, 1, of);
            if (sent) fwrite(&st, sizeof st, 1, of);
        } else return 3;
    }
    if (refused) { fclose(of); return refused; }
    const state_t &s = q.s;
    const int32_t iv[11] = {s.points, s.nsamp, s.exponent, s.msk_mode, s.msk_baud, s.draw, s.display_mode, s.maN, s.maNsend, s.ring[0], s.ring[1]};
    const float fv[6] = {s.gain, s.fs, s.pll_bandwidth, s.cma_re, s.cma_im, s.ama};
    fwrite(iv, sizeof iv, 1, of);
    fwrite(fv, sizeof fv, 1, of);
    for (int w = 0; w < 3; w++) {
        const pll_t &p = s.pll[w];
        const float pv[7] = {p.fs, p.fc, p.df, p.phase, p.b0, p.b1, p.ud};
        fwrite(pv, sizeof pv, 1, of);
    }
    fwrite(q.iq, sizeof q.iq, 1, of);
    fwrite(q.plot, sizeof q.plot, 1, of);
    fwrite(q.map, sizeof q.map, 1, of);
    fclose(of);
    return 0;
}
