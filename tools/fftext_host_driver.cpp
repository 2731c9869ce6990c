// Host driver of csrc/kg_fftext.h (tests/fftext_common.py compiles it with g++ -O2 -ffp-contract=off, the reference's flags): the FFT
// extension's commands, schedule, sums, rows and limiter, with the modes, the script language and the output layouts of
// tools/ref/ref_fftext_main.cpp.
//   fftext_host_driver script  script.txt pool.bin out.bin
//   fftext_host_driver limiter clocks.bin out.bin
// Exit status 10 + the refusal's number (11: the period of an integ block, 12: bins outside int, 13: a run outside -1 .. 2) when
// kg_fftext.h refuses what the reference leaves undefined; out.bin then holds what came before.
#include "../flydog_sdr_gps_amd/csrc/kg_fftext.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace kg_fftext_cf;

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

enum { MODE_QAM = 15 };                                                 // rx/mode.h:69-70

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: %s script|limiter ...\n", argv[0]); return 2; }
    state_t e;
    init(e);
    static float pwr[MAX_BINS][WIDTH];
    static int ncma[MAX_BINS];
    const size_t SPEC = WIDTH * 2 * sizeof(float);
    if (!strcmp(argv[1], "script") && argc == 5) {
        FILE *sf = fopen(argv[2], "r"), *of = fopen(argv[4], "wb");
        if (!sf || !of) return 2;
        const std::vector<unsigned char> pool = slurp(argv[3]);
        double rate = 0;
        bool registered = false;
        char line[256];
        unsigned char fft[WIDTH];
        while (fgets(line, sizeof line, sf)) {
            line[strcspn(line, "\n")] = 0;
            const char op = line[0];
            if (op == 'R') {
                if (sscanf(line + 1, "%lf", &rate) != 1) return 3;
            } else if (op == 'S') {
                int run, sam, mode;
                if (sscanf(line + 1, "%d %d %d", &run, &sam, &mode) != 3) return 3;
                if (cmd_run(e, run, sam != 0, mode == MODE_QAM)) { fclose(of); return 13; }
                registered = run != FUNC_OFF;
            } else if (op == 'I') {
                double t;
                if (sscanf(line + 1, "%lf", &t) != 1) return 3;
                cmd_itime(e, t);
            } else if (op == 'C') {
                cmd_clear(e);
            } else if (op == 'B') {
                int inst;
                unsigned long k;
                if (sscanf(line + 1, "%d %lu", &inst, &k) != 2 || (k + 1) * SPEC > pool.size()) return 3;
                int bin = 0, did_reset = 0, sent = 0;
                if (registered) {
                    sent = block(e, inst, rate, &bin, &did_reset);
                    if (sent < 0) { fclose(of); return 10 - sent; }
                    if (did_reset) { memset(pwr, 0, sizeof pwr); memset(ncma, 0, sizeof ncma); }
                }
                fwrite(&sent, 4, 1, of);
                if (sent) {
                    body(e, (const float *) (pool.data() + k * SPEC), pwr[bin], &ncma[bin], fft);
                    fwrite(&bin, 4, 1, of);
                    fwrite(fft, 1, WIDTH, of);
                }
            } else if (op != 0 && op != '#') return 3;
        }
        const int iv[4] = {e.run, e.instance, e.bins, e.reset};
        const float fv[2] = {e.fft_scale, e.spectrum_scale};
        const double dv[3] = {e.fi, e.fft_sec, e.time};
        fwrite(iv, sizeof iv, 1, of);
        fwrite(fv, sizeof fv, 1, of);
        fwrite(dv, sizeof dv, 1, of);
        fwrite(ncma, sizeof ncma, 1, of);
        fwrite(pwr, sizeof pwr, 1, of);
        fclose(of);
        return 0;
    }
    if (!strcmp(argv[1], "limiter")) {
        const std::vector<unsigned char> in = slurp(argv[2]);
        FILE *of = fopen(argv[3], "wb");
        if (!of || in.size() % 4) return 2;
        cmd_run(e, FUNC_SPEC, false, false);
        for (size_t k = 0; k < in.size() / 4; k++) {
            uint32_t now;
            memcpy(&now, in.data() + 4 * k, 4);
            const int sent = due(e, now);
            fwrite(&sent, 4, 1, of);
            fwrite(&e.last_ms, 4, 1, of);
        }
        fclose(of);
        return 0;
    }
    return 2;
}
