// Developer and test tool: csrc/kg_cw.h compiled for the HOST with the reference's flags (g++ -O2 -ffp-contract=off), reading the
// scripts of tests/cw_common.py and writing what tools/ref/ref_cw_main.cpp writes (its header comment has the formats; the eight
// trailing counters are zeros here).  A refused command ends the run with 20 - (the refusal's code of kg_cw.h); with -k it is skipped
// and the run goes on, which is how tests/test_cw_cpu.py shows that a refusal changes nothing.
//
//   cw_host_driver [-k] script.txt pool.bin out.bin
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../flydog_sdr_gps_amd/csrc/kg_cw.h"

using namespace kg_cw_cf;

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

int main(int argc, char **argv)
{
    bool keep_on = false;
    if (argc > 1 && !strcmp(argv[1], "-k")) { keep_on = true; argv++; argc--; }
    if (argc != 4) { fprintf(stderr, "usage: %s [-k] script.txt pool.bin out.bin\n", argv[0]); return 2; }
    FILE *sf = fopen(argv[1], "r"), *of = fopen(argv[3], "wb");
    if (!sf || !of) return 2;
    std::vector<unsigned char> pool = slurp(argv[2]);
    const size_t npool = pool.size() / sizeof(int16_t);
    state_t *q = (state_t *) calloc(1, sizeof(state_t));                 // begins zeroed, as the static cw_decoder[] does
    if (!q) return 2;
    std::vector<ev_t> evs((size_t) max_events(1));
    double nom = 0, srate = 0;                                          // what the last start gave: `SET cw_wpm=` reads them again
    uint32_t now = 0;
    char line[256];
    while (fgets(line, sizeof line, sf)) {
        line[strcspn(line, "\n")] = 0;
        const char op = line[0];
        int rc = 0, a = 0, b = 0;
        if (op == 0 || op == '#') {
        } else if (op == 'S') {
            double n, r;
            if (sscanf(line + 1, "%d %lf %lf", &a, &n, &r) != 3) return 3;
            rc = start_check(a, n, r);
            if (rc == 0) {
                nom = n; srate = r;
                cmd_init(*q, 0, a, (int32_t) nom, srate);
                q->started = 1;
            }
        } else if (op == 'W') {
            if (sscanf(line + 1, "%d %d", &a, &b) != 2) return 3;
            if (nom == 0) rc = REFUSED_NOT_STARTED;
            else if (a < 0) rc = REFUSED_WPM;
            else if (a == 0) rc = start_check(b, nom, srate);
            if (rc == 0) cmd_init(*q, a, b, (int32_t) nom, srate);
        } else if (op == 'P') {
            if (sscanf(line + 1, "%d", &a) != 1) return 3;
            rc = pboff_check(q->sampling_freq, q->blocksize, (uint32_t) a);
            if (rc == 0) cmd_pboff(*q, (uint32_t) a);
        } else if (op == 'C') {
            if (sscanf(line + 1, "%d", &a) != 1) return 3;
            cmd_wsc(*q, a);
        } else if (op == 'A') {
            if (sscanf(line + 1, "%d", &a) != 1) return 3;
            cmd_auto_threshold(*q, a);
        } else if (op == 'H') {
            if (sscanf(line + 1, "%d", &a) != 1) return 3;
            cmd_threshold(*q, a);
        } else if (op == 'T') {
            q->started = 0;
        } else if (op == 'N') {
            unsigned long n;
            if (sscanf(line + 1, "%lu", &n) != 1) return 3;
            now = (uint32_t) n;
        } else if (op == 'B') {
            unsigned long off;
            if (sscanf(line + 1, "%lu", &off) != 1 || off + BLK > npool) return 3;
            sink_t k = {evs.data(), 0, (int32_t) evs.size(), 0, 0, 0};
            host_block(*q, (const int16_t *) pool.data() + off, now, k);
            if (k.overflow) return 9;                                   // the bound of kg_cw.h does not hold
            fwrite(&k.n, 4, 1, of);
            if (k.n) fwrite(evs.data(), sizeof(ev_t), (size_t) k.n, of);
        } else return 3;
        if (rc != 0 && !keep_on) return 20 - rc;
    }
    fwrite(q, sizeof *q, 1, of);
    const int32_t tail[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    fwrite(tail, sizeof tail, 1, of);
    fclose(of);
    free(q);
    return 0;
}
