// Host driver of csrc/kg_nbw.h (tests/test_nbw_cpu.py compiles it with g++ -O2 -ffp-contract=off): runs the scenarios of
// tests/golden/nbw_ref.npz with the script language and the output layout of tools/ref/ref_nbw_main.cpp, with the command semantics
// that kg_rxbank_nbw_select / kg_rxbank_set_nb_algo / _set_nb_enable / _set_nb_param and kg_post_nbw_init / kg_post_set_nbw /
// kg_post_reset implement (one channel).  Exit status 6: a command the library refuses (the stage on an unusable vector).
//   nbw_host_driver script.txt in.bin out.bin st.bin tr.bin
// tr.bin: per block that ran the stage, int32 hits; float largest |sample| handed to the int16 conversion (inf for a NaN).
#include "../flydog_sdr_gps_amd/csrc/kg_nbw.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace kg_nbw;

static state_t st;                // the zeroed static nb_Wild[ch]

int main(int argc, char **argv)
{
    if (argc != 6) { fprintf(stderr, "usage: %s script in.bin out.bin st.bin tr.bin\n", argv[0]); return 2; }
    FILE *sf = fopen(argv[1], "r"), *inf = fopen(argv[2], "rb"), *outf = fopen(argv[3], "wb"), *stf = fopen(argv[4], "wb"),
         *trf = fopen(argv[5], "wb");
    if (!sf || !inf || !outf || !stf || !trf) return 2;
    int algo = 0, en[4] = {0, 0, 0, 0};
    float param[4][kg_nr::NPARAMS];
    memset(param, 0, sizeof param);
    static short buf[BLOCK];
    char line[1024];
    while (fgets(line, sizeof line, sf)) {
        const char op = line[0];
        if (op == 'A') {
            int a;
            if (sscanf(line + 1, "%d", &a) != 1) return 3;
            algo = a;
            memset(en, 0, sizeof en);
            st.on = 0;
        } else if (op == 'E') {
            int t, e;
            if (sscanf(line + 1, "%d %d", &t, &e) != 2 || t < 0 || t > 3) return 3;
            if (t == 0 && algo == 2) {
                if (e && !usable(st)) return 6;
                st.on = e != 0;
            }
            en[t] = e;
        } else if (op == 'P') {
            int t, p;
            float v;
            if (sscanf(line + 1, "%d %d %f", &t, &p, &v) != 3 || t < 0 || t > 3 || p < 0 || p >= kg_nr::NPARAMS) return 3;
            float vec[kg_nr::NPARAMS];
            memcpy(vec, param[t], sizeof vec);
            vec[p] = v;
            if (t == 0 && algo == 2) {
                state_t n = st;
                init_params(n, vec);
                if (st.on && !usable(n)) return 6;
                const int on = st.on;
                memset(&st, 0, sizeof st);                              // nb_Wild_init's memset, the history included
                init_params(st, vec);
                st.on = on;
            }
            memcpy(param[t], vec, sizeof vec);
        } else if (op == 'C') {
            algo = 0;
            memset(en, 0, sizeof en);
            memset(param, 0, sizeof param);
            st.on = 0;                                                  // memset(s): nb_Wild[ch] stays
        } else if (op == 'B') {
            int n, stereo;
            if (sscanf(line + 1, "%d %d", &n, &stereo) != 2 || n != BLOCK) return 3;
            if (fread(buf, sizeof(short), n, inf) != (size_t) n) return 4;
            if (!stereo && st.on) {
                trace_t tr;
                process(st, buf, buf, &tr);
                fwrite(&tr.hits, sizeof tr.hits, 1, trf);
                fwrite(&tr.max_abs, sizeof tr.max_abs, 1, trf);
            }
            fwrite(buf, sizeof(short), n, outf);
        } else if (op == 'S') {
            const int iv[4] = {st.taps, st.impulse_samples, algo, en[0]};
            fwrite(iv, sizeof iv, 1, stf);
            fwrite(&st.thresh, sizeof(float), 1, stf);
            fwrite(st.hist, sizeof(float), HIST_MAX, stf);
        } else if (op != '\n' && op != '#') return 3;
    }
    fclose(outf); fclose(stf); fclose(trf);
    return 0;
}
