// Developer and test tool: csrc/kg_fax.h compiled for the HOST with the reference's flags (g++ -O2 -ffp-contract=off), reading the
// scripts of tests/fax_common.py and writing what tools/ref/ref_fax_main.cpp writes (its header comment has the formats).  A refused
// command ends the run with 20 - (the refusal's code of kg_fax.h); with -k it is skipped and the run goes on, which is how
// tests/test_fax_cpu.py shows that a refusal changes nothing.
//
//   fax_host_driver [-k] script.txt pool.bin out.bin
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../flydog_sdr_gps_amd/csrc/kg_fax.h"

using namespace kg_fax_cf;

static std::vector<unsigned char> sent;
static int nlines;
static void on_line(void *, const rec_t *r, const uint8_t *row, int nbytes)
{
    sent.insert(sent.end(), (const unsigned char *) r, (const unsigned char *) r + sizeof *r);
    if (row) sent.insert(sent.end(), row, row + nbytes);
    nlines++;
}

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
    full_t *q = (full_t *) calloc(1, sizeof(full_t));                    // begins zeroed
    if (!q) return 2;
    double cur_srate = 0;
    bool configured = false;
    char line[256];
    while (fgets(line, sizeof line, sf)) {
        line[strcspn(line, "\n")] = 0;
        const char op = line[0];
        int rc = 0;
        if (op == 'C') {
            int lpm, w, car, dev, bw, hdr, ph, as, dbg, spl;
            double nom, sr;
            if (sscanf(line + 1, "%d %d %d %d %d %d %d %d %d %lf %lf", &lpm, &w, &car, &dev, &bw, &hdr, &ph, &as, &dbg, &nom, &sr) != 11) return 3;
            rc = start_check(lpm, w, dev, bw, nom, sr, &spl);
            if (rc == 0) {
                full_start(*q, lpm, w, car, dev, bw, hdr, ph, as, dbg, nom, sr);
                cur_srate = sr;
                configured = true;
            }
        } else if (op == 0 || op == '#') {
        } else if (op == 'R') {
            double sr;
            if (sscanf(line + 1, "%lf", &sr) != 1) return 3;
            if (configured && !rate_ok(q->s, sr)) rc = REFUSED_RATE;
            else cur_srate = sr;
        } else if (op == 'H') {
            float sh;
            if (sscanf(line + 1, "%f", &sh) != 1) return 3;
            if (!shift_ok(sh)) rc = REFUSED_SHIFT;
            else q->shift = sh;
        } else if (op == 'T') {
            q->started = 0;
            q->shift = 0;
        } else if (op == 'B') {
            unsigned long off;
            if (sscanf(line + 1, "%lu", &off) != 1 || off + BLK > npool) return 3;
            sent.clear();
            nlines = 0;
            full_block(*q, (const int16_t *) pool.data() + off, cur_srate, 0, on_line, nullptr);
            fwrite(&nlines, 4, 1, of);
            if (!sent.empty()) fwrite(sent.data(), 1, sent.size(), of);
        } else return 3;
        if (rc != 0 && !keep_on) return 20 - rc;
    }
    if (!configured) return 5;
    const state_t &s = q->s;
    float fir[2][TAPS];
    int32_t current;
    fir_circular(s, fir, &current);
    const double d[10] = {s.nom, s.frac, s.frac_prev, s.ratio, s.fi, s.lineIncrFrac, s.lineIncrAcc, s.lineBlend, s.carrier, s.deviation};
    const int32_t n[20] = {s.lpm, s.imagewidth, s.bandwidth, s.include_headers, s.use_phasing, s.autostop, s.autostopped, s.debug, s.skip_header_detection, s.spl,
                           s.skip, s.samp_idx, s.lasttype, s.typecount, s.imageline, s.phasingLinesLeft, s.phasingSkipData, s.have_phasing, current, q->started};
    const float pq[2] = {s.Iprev, s.Qprev};
    fwrite(d, sizeof d, 1, of); fwrite(n, sizeof n, 1, of); fwrite(pq, sizeof pq, 1, of);
    fwrite(fir, sizeof fir, 1, of);
    fwrite(s.phasingPos, sizeof s.phasingPos, 1, of);
    int32_t tail[2] = {0, 0};
    memcpy(&tail[0], &q->shift, 4);
    fwrite(tail, sizeof tail, 1, of);
    fwrite(q->samples, 2, (size_t) s.spl, of);
    fwrite(q->demod, 1, (size_t) s.spl, of);
    std::vector<unsigned char> prev((size_t) s.imagewidth, 0);
    if (s.imageline != 0) memcpy(prev.data(), q->prev, (size_t) s.imagewidth);
    fwrite(prev.data(), 1, prev.size(), of);
    fwrite(q->out, 1, (size_t) s.imagewidth, of);
    fclose(of);
    free(q);
    return 0;
}
