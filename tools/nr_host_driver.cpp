// Host driver of csrc/kg_nr.h (tests/test_nr_cpu.py compiles it with g++ -O2 -ffp-contract=off): runs the unit scenarios of
// tests/golden/nr_ref.npz with the same script language and output layout as tools/ref/ref_nr_main.cpp, with the `SET nr` command
// semantics that kg_post_set_nr_algo / _enable / _param implement (one channel).
//   nr_host_driver script.txt in.bin out.bin
#include "../flydog_sdr_gps_amd/csrc/kg_nr.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace kg_nr;

static anr_t anr[2];
static float anr_d[2][ANR_DLINE], anr_w[2][ANR_DLINE];
static lms_t lms[2];
static float lms_ring[2][LMS_RING], lms_c[2][LMSLEN];

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s script in.bin out.bin\n", argv[0]); return 2; }
    FILE *sf = fopen(argv[1], "r"), *inf = fopen(argv[2], "rb"), *outf = fopen(argv[3], "wb");
    if (!sf || !inf || !outf) return 2;
    int algo = 0, en[2] = {0, 0};
    float param[2][NPARAMS];
    memset(param, 0, sizeof param);
    static short buf[4096];
    char line[1024];
    while (fgets(line, sizeof line, sf)) {
        const char op = line[0];
        if (op == 'A') {
            if (sscanf(line + 1, "%d", &algo) != 1) return 3;
            en[0] = en[1] = 0;
        } else if (op == 'E') {
            int t, e;
            if (sscanf(line + 1, "%d %d", &t, &e) != 2 || t < 0 || t > 1) return 3;
            en[t] = e;
        } else if (op == 'P') {
            int t, p;
            float v;
            if (sscanf(line + 1, "%d %d %f", &t, &p, &v) != 3 || t < 0 || t > 1 || p < 0 || p >= NPARAMS) return 3;
            param[t][p] = v;
            if (algo == 1) {
                if (!anr_params_ok(param[t])) return 6;
                anr_init(anr[t], anr_d[t], anr_w[t], param[t]);
            } else if (algo == 2) {
                if (!lms_params_ok(param[t])) return 6;
                lms_init(lms[t], lms_ring[t], lms_c[t], t, param[t]);
            }
        } else if (op == 'C') {
            algo = 0; en[0] = en[1] = 0;
            memset(param, 0, sizeof param);
        } else if (op == 'B') {
            int n, stereo;
            if (sscanf(line + 1, "%d %d", &n, &stereo) != 2 || n < 1 || n > 4096) return 3;
            if (fread(buf, sizeof(short), n, inf) != (size_t) n) return 4;
            if (!stereo) {
                if (algo == 1) {
                    if (en[AUTONOTCH]) anr_filter(anr[1], anr_d[1], anr_w[1], AUTONOTCH, n, buf, buf);
                    if (en[DENOISE]) anr_filter(anr[0], anr_d[0], anr_w[0], DENOISE, n, buf, buf);
                } else if (algo == 2) {
                    if (en[AUTONOTCH]) lms_filter(lms[1], lms_ring[1], lms_c[1], n, buf, buf);
                    if (en[DENOISE]) lms_filter(lms[0], lms_ring[0], lms_c[0], n, buf, buf);
                }
            }
            fwrite(buf, sizeof(short), n, outf);
        } else if (op == 'S') {
            for (int t = 0; t < 2; t++) {
                const int iv[6] = {anr[t].in_idx, anr[t].taps, anr[t].delay, lms[t].dlp, lms[t].dlen, lms[t].nr_type};
                const float fv[2] = {anr[t].lidx, anr[t].ngamma};
                fwrite(iv, sizeof iv, 1, outf);
                fwrite(fv, sizeof fv, 1, outf);
                fwrite(anr_w[t], sizeof(float), ANR_DLINE, outf);
                fwrite(lms_c[t], sizeof(float), LMSLEN, outf);
            }
        } else if (op != '\n' && op != '#') return 3;
    }
    fclose(outf);
    return 0;
}
