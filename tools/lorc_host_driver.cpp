// Host driver of csrc/kg_lorc.h (tests/lorc_common.py compiles it with g++ -O2 -ffp-contract=off, the reference's flags): the Loran-C
// extension's commands, schedule, averages and rows, with the script language and the output layout of tools/ref/ref_lorc_main.cpp.
//   lorc_host_driver [-r] [-k] script.txt pool.bin out.bin     -r: loran_c_data through the run decomposition (plan_stretch, as the
//                                                          kernel walks it) instead of sample by sample with one fmod a sample;
//                                                          -k: a refused command or block is passed over, not the script's end
//   lorc_host_driver selftest                             the run decomposition against the per-sample schedule, no samples involved
// Exit status 10 + the refusal's number (11: the Loran channel, 12: the gri, 13: nbucket >= 1199, 14: an offset before a GRI, 15: the
// rule, 16: a push without a GRI, 17: EMA below 1, 18: IIR negative or not finite, 19: a command or block before `N`) when kg_lorc.h
// refuses; out.bin then holds what came before.
#include "../flydog_sdr_gps_amd/csrc/kg_lorc.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace kg_lorc_cf;

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
static void emit(void *, int samp, int ch, int cmd, const unsigned char *bytes, int nbytes)
{
    const int32_t h[4] = {samp, ch, cmd, nbytes};
    sent_rows.insert(sent_rows.end(), (const unsigned char *) h, (const unsigned char *) h + 16);
    sent_rows.insert(sent_rows.end(), bytes, bytes + nbytes);
    nrows++;
}

// One configuration of the self test: n samples of one channel, per sample (bn, emit, zero, navgs) from bucket() + first_sample()
// against the runs of run_walk() laid out sample by sample, and the scalars behind both.
static int selftest_one(const char *name, double srate, int i_srate, int gri, int algo, double param, uint32_t samp0, int offset, int n, int chunk)
{
    state_t a;
    memset(&a, 0, sizeof a);
    cmd_init(a, srate, i_srate);
    if (cmd_gri(a, 0, gri) || cmd_avg_algo(a, 0, algo) || cmd_avg_param(a, 0, param)) return 1;
    cmd_start(a);
    a.ch[0].samp = samp0;
    a.ch[0].offset = offset;
    state_t b = a;
    long nruns = 0, nemit = 0, nzero = 0, wraps = 0;
    std::vector<int32_t> want(4 * (size_t) chunk), got(4 * (size_t) chunk);
    for (int done = 0; done < n; done += chunk) {
        const int m = n - done < chunk ? n - done : chunk;
        for (int i = 0; i < m; i++) {
            chan_t &c = a.ch[0];
            const int bn = bucket(c);
            int em, zero;
            wraps += c.samp == 0xffffffffu;
            first_sample(a, c, bn, &em, &zero);
            want[4 * i] = bn; want[4 * i + 1] = em; want[4 * i + 2] = zero; want[4 * i + 3] = (int32_t) c.navgs;
        }
        int at = 0, bad = 0;
        run_walk(b, b.ch[0], m, [&](const run_t &r) {
            if (r.start != at || r.len < 1) bad = 1;
            for (int k = 0; k < r.len && at < m; k++, at++) {
                got[4 * at] = r.bn0 + k; got[4 * at + 1] = k ? 0 : r.emit; got[4 * at + 2] = k ? 0 : r.zero; got[4 * at + 3] = (int32_t) r.navgs;
            }
            nruns++; nemit += r.emit; nzero += r.zero;
        });
        if (bad || at != m || memcmp(want.data(), got.data(), sizeof(int32_t) * 4 * (size_t) m) || memcmp(&a, &b, sizeof a)) {
            printf("%s: the runs differ from the per-sample schedule in samples %d .. %d\n", name, done, done + m);
            return 1;
        }
    }
    printf("%s: %d samples, %ld runs, %ld rows, %ld clears, %ld wraps of samp, nbucket %u, samp_per_GRI %.6f\n", name, n, nruns, nemit, nzero, wraps,
           a.ch[0].nbucket, a.ch[0].samp_per_GRI);
    return 0;
}

static int selftest()
{
    int bad = 0;
    // samp < offset at the start: the unsigned difference starts 700 below 2^32 and wraps
    bad |= selftest_one("below_offset", 12000.0, 12000, 7980, AVG_CMA, 3, 0, 700, 600000, 4096);
    // the 2^32 wrap of samp, with an offset so that the difference wraps elsewhere
    bad |= selftest_one("samp_wrap", 12000.0, 12000, 9960, AVG_CMA, 2, 0xffffffffu - 300000u, 333, 600000, 512);
    // a halved GRI at a non-integer rate
    bad |= selftest_one("halved_12001.3", 12001.3 * 20250 / 12000, 20250, 7980, AVG_EMA, 8, 0xffffffffu - 100000u, 5, 500000, 170);
    bad |= selftest_one("rate_12001.3", 12001.3, 600, 8970, AVG_IIR, 0.001, 17, 1100, 500000, 512);
    // nbucket 1 and 2: a run a sample, or nearly
    bad |= selftest_one("nbucket_1", 12000.0, 600, 8, AVG_CMA, 2, 0, 0, 100000, 512);
    bad |= selftest_one("nbucket_2", 12000.0, 600, 9, AVG_CMA, 2, 0xffffffffu - 50000u, 1, 100000, 512);
    printf(bad ? "FAILED\n" : "OK\n");
    return bad;
}

static void put_state(FILE *of, const full_t &q)
{
    const state_t &s = q.s;
    const int32_t head[2] = {(int32_t) s.i_srate, s.redraw_legend};
    fwrite(head, sizeof head, 1, of);
    fwrite(&s.srate, 8, 1, of);
    for (int ch = 0; ch < NCH; ch++) {
        const chan_t &c = s.ch[ch];
        const uint32_t u[6] = {c.gri, c.samp, c.nbucket, c.dsp_samps, c.avg_samps, c.navgs};
        const float f[2] = {c.gain, q.max[ch]};
        const int32_t i1[2] = {c.offset, c.avg_algo}, i2[2] = {c.avg_param_i, c.restart};
        fwrite(u, sizeof u, 1, of); fwrite(&c.samp_per_GRI, 8, 1, of); fwrite(f, sizeof f, 1, of); fwrite(i1, sizeof i1, 1, of);
        fwrite(&c.avg_param_f, 8, 1, of); fwrite(i2, sizeof i2, 1, of);
    }
    fwrite(q.avg, sizeof q.avg, 1, of);
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "selftest")) return selftest();
    bool by_runs = false, keep_on = false;
    while (argc > 4 && argv[1][0] == '-') {
        if (!strcmp(argv[1], "-r")) by_runs = true;
        else if (!strcmp(argv[1], "-k")) keep_on = true;
        else break;
        argv++; argc--;
    }
    if (argc != 4) { fprintf(stderr, "usage: %s [-r] [-k] script.txt pool.bin out.bin | selftest\n", argv[0]); return 2; }
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
        int a = 0, b = 0, rc = 0;
        double v;
        if (op == 'N') {
            if (sscanf(line + 1, "%lf %d", &v, &a) != 2) return 3;
            const int started = q.s.started;
            memset(&q, 0, sizeof q);
            q.s.started = started;
            cmd_init(q.s, v, a);
        } else if (op == 0 || op == '#') {
        } else if (!q.s.inited) {
            if (!keep_on) refused = 19;
        } else if (op == 'I') {
            if (sscanf(line + 1, "%d %d", &a, &b) != 2) return 3;
            rc = cmd_gri(q.s, a, b);
        } else if (op == 'O') {
            if (sscanf(line + 1, "%d %d", &a, &b) != 2) return 3;
            rc = cmd_offset(q.s, a, b);
        } else if (op == 'G') {
            if (sscanf(line + 1, "%d %d", &a, &b) != 2) return 3;
            rc = cmd_gain(q.s, a, b);
        } else if (op == 'A') {
            if (sscanf(line + 1, "%d %d", &a, &b) != 2) return 3;
            rc = cmd_avg_algo(q.s, a, b);
        } else if (op == 'P') {
            if (sscanf(line + 1, "%d %lf", &a, &v) != 2) return 3;
            rc = cmd_avg_param(q.s, a, v);
        } else if (op == 'S') {
            cmd_start(q.s);
        } else if (op == 'T') {
            cmd_stop(q.s);
        } else if (op == 'B') {
            int ns;
            unsigned long off;
            if (sscanf(line + 1, "%d %lu", &ns, &off) != 2 || ns < 1 || ns > MAX_NS || off + ns > npool) return 3;
            sent_rows.clear();
            nrows = 0;
            if (q.s.started) {
                const float *x = (const float *) (pool.data() + 8 * off);
                if ((rc = push_check(q.s)) != 0) { if (!keep_on) { refused = 10 - rc; break; } }
                else if (by_runs) data_by_runs(q, ns, x, emit, nullptr);
                else data_per_sample(q, ns, x, emit, nullptr);
            }
            fwrite(&nrows, 4, 1, of);
            if (!sent_rows.empty()) fwrite(sent_rows.data(), 1, sent_rows.size(), of);
        } else return 3;
        if (rc && !keep_on) refused = 10 - rc;
    }
    if (refused) { fclose(of); return refused; }
    put_state(of, q);
    fclose(of);
    return 0;
}
