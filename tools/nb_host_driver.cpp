// Host driver of flydog_sdr_gps_amd/csrc/kg_nb.h (tests/test_nb_cpu.py builds it with g++ -O2 -ffp-contract=off): the script
// language of tools/ref/ref_nb_main.cpp, answered by kg_nb.h's serial restatement instead of the reference's CNoiseProc.  Also
//   nb_host_driver --setup rate gate th   -> one line: status M D G ratio(%a) of kg_nbk::setup on a fresh blanker
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../flydog_sdr_gps_amd/csrc/kg_nb.h"

struct blanker {
    kg_nbk::st s{};
    bool was = false;
    std::vector<float> mag = std::vector<float>(kg_nbk::MAG_RING, 0.0f), dly = std::vector<float>(2 * kg_nbk::DLY_RING, 0.0f);
    int setup(float rate, float gate, float th)
    {
        float p[kg_nbk::NPARAMS] = {gate, th};
        const int r = kg_nbk::setup(s, was, rate, p);
        if (r == kg_nbk::SETUP_OK) {
            was = true;
            std::fill(mag.begin(), mag.end(), 0.0f);
            std::fill(dly.begin(), dly.end(), 0.0f);
        }
        return r;
    }
    void dump(FILE *f) const
    {
        const int iv[6] = {s.mptr, s.dptr, s.cnt, s.M, s.D, s.G};
        const float fv[2] = {s.ratio, s.sum};
        fwrite(iv, sizeof iv, 1, f);
        fwrite(fv, sizeof fv, 1, f);
    }
};

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "--setup")) {
        blanker b;
        const int r = b.setup(strtof(argv[2], nullptr), strtof(argv[3], nullptr), strtof(argv[4], nullptr));
        printf("%d %d %d %d %a\n", r, b.s.M, b.s.D, b.s.G, (double) b.s.ratio);
        return 0;
    }
    if (argc != 4) { fprintf(stderr, "usage: %s script in.bin out.bin | --setup rate gate th\n", argv[0]); return 2; }
    FILE *sf = fopen(argv[1], "r"), *inf = fopen(argv[2], "rb"), *outf = fopen(argv[3], "wb");
    if (!sf || !inf || !outf) { fprintf(stderr, "cannot open files\n"); return 2; }
    blanker snd, wf;
    std::vector<float> buf(2 << 16);
    char line[1024], a[64], b[64], c[64];
    while (fgets(line, sizeof line, sf)) {
        const char op = line[0];
        if (op == 'U') {
            if (sscanf(line + 1, "%63s %63s %63s", a, b, c) != 3) return 3;
            if (snd.setup(strtof(a, nullptr), strtof(b, nullptr), strtof(c, nullptr))) return 6;
        } else if (op == 'B') {
            int n;
            if (sscanf(line + 1, "%d", &n) != 1 || n < 0 || n > (1 << 16)) return 3;
            if (fread(buf.data(), 8, n, inf) != (size_t) n) return 4;
            kg_nbk::process(snd.s, snd.mag.data(), snd.dly.data(), n, buf.data(), buf.data());
            fwrite(buf.data(), 8, n, outf);
        } else if (op == 'W') {
            if (sscanf(line + 1, "%63s %63s", b, c) != 2) return 3;
            if (wf.setup((float) kg_nbk::WF_NSAMPS, strtof(b, nullptr), strtof(c, nullptr))) return 6;
        } else if (op == 'F') {
            if (fread(buf.data(), 8, kg_nbk::WF_NSAMPS, inf) != kg_nbk::WF_NSAMPS) return 4;
            kg_nbk::one_shot(wf.s, wf.mag.data(), wf.dly.data(), buf.data(), buf.data());
            fwrite(buf.data(), 8, kg_nbk::WF_NSAMPS, outf);
        } else if (op == 'S') {
            snd.dump(outf);
        } else if (op == 'T') {
            wf.dump(outf);
        } else if (op != '\n' && op != '#') return 3;
    }
    fclose(outf);
    return 0;
}
