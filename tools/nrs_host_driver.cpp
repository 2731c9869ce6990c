// Host driver of csrc/kg_nrs.h (tests/test_nrs_cpu.py compiles it with g++ -O2 -ffp-contract=off): runs the scenarios of
// tests/golden/nrs_ref.npz with the script language and the output layout of tools/ref/ref_nrs_main.cpp, with the command semantics
// that kg_post_nrs_select / kg_post_set_nr_param / kg_post_nrs_passband / kg_post_reset implement (one channel).  Exit status 6: a
// command the library refuses (a passband on which the reference would index outside its arrays).
//   nrs_host_driver snd_rate script.txt in.bin out.bin st.bin tr.bin
// tr.bin: per block that ran the stage, int32 NN of its phase-3 frames in order (0-padded), bins with pslp > psthr, first_time, and
// (more than the reference's harness can see) the number of frames with a NaN power_ratio.
#include "../flydog_sdr_gps_amd/csrc/kg_nrs.h"
#include "../flydog_sdr_gps_amd/csrc/kg_tables.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace kg_nrs;

static state_t st;                // the zeroed static nr_spectral[ch]
static bool inited;

int main(int argc, char **argv)
{
    if (argc != 7) { fprintf(stderr, "usage: %s snd_rate script in.bin out.bin st.bin tr.bin\n", argv[0]); return 2; }
    const int snd_rate = atoi(argv[1]);
    FILE *sf = fopen(argv[2], "r"), *inf = fopen(argv[3], "rb"), *outf = fopen(argv[4], "wb"), *stf = fopen(argv[5], "wb"),
         *trf = fopen(argv[6], "wb");
    if (!sf || !inf || !outf || !stf || !trf) return 2;
    const rate_t rt = rate_consts(snd_rate);
    int algo = 0;
    float param[2][kg_nr::NPARAMS], norm_lo = 0, norm_hi = 0;
    memset(param, 0, sizeof param);
    static short buf[512];
    char line[1024];
    while (fgets(line, sizeof line, sf)) {
        const char op = line[0];
        if (op == 'A') {
            int a;
            if (sscanf(line + 1, "%d", &a) != 1) return 3;
            if (a == 3) {
                int lo, hi;
                vad_bins(norm_lo, norm_hi, snd_rate, lo, hi);
                if (!vad_ok(lo, hi)) return 6;
            }
            algo = a;
        } else if (op == 'E') {
            // the enables are not consulted under NR_SPECTRAL (rx_sound.cpp:945-947)
        } else if (op == 'P') {
            int t, p;
            float v;
            if (sscanf(line + 1, "%d %d %f", &t, &p, &v) != 3 || t < 0 || t > 1 || p < 0 || p >= kg_nr::NPARAMS) return 3;
            param[t][p] = v;
            if (algo == 3) {
                if (!inited) { inited = true; init_first(st); }
                init_params(st.par, param[t]);
            }
        } else if (op == 'M') {
            double lo, hi;
            if (sscanf(line + 1, "%lf %lf", &lo, &hi) != 2) return 3;
            float nl, nh;
            int vl, vh;
            norm_passband(lo, hi, nl, nh);
            vad_bins(nl, nh, snd_rate, vl, vh);
            if (algo == 3 && !vad_ok(vl, vh)) return 6;
            norm_lo = nl; norm_hi = nh;
            st.vad_lo = vl; st.vad_hi = vh;
        } else if (op == 'C') {
            algo = 0;
            memset(param, 0, sizeof param);
            norm_lo = norm_hi = 0;                                      // memset(s): norm_locut / norm_hicut too
            vad_bins(norm_lo, norm_hi, snd_rate, st.vad_lo, st.vad_hi);
        } else if (op == 'B') {
            int n, stereo;
            if (sscanf(line + 1, "%d %d", &n, &stereo) != 2 || n != 512) return 3;
            if (fread(buf, sizeof(short), n, inf) != (size_t) n) return 4;
            if (!stereo && algo == 3) {
                trace_t tr;
                process(st, rt, KG_NRS_TW.v, KG_NRS_WIN.v, buf, buf, &tr);
                int over = 0;
                for (int b = 0; b < FFT_HALF; b++) over += st.pslp[b] > (float) 0.99;
                const int rec[5] = {tr.nn[0], tr.nn[1], over, st.first_time, tr.nan_ratio};
                fwrite(rec, sizeof rec, 1, trf);
            }
            fwrite(buf, sizeof(short), n, outf);
        } else if (op == 'S') {
            const int iv[2] = {st.first_time, st.init_counter};
            const float fv[12] = {st.par.final_gain, st.par.alpha, st.par.asnr, st.par.xih1r, st.par.pfac,
                                  inited ? rt.tinc : 0, inited ? rt.tax : 0, inited ? rt.tap : 0, inited ? rt.ax : 0, inited ? rt.ap : 0,
                                  norm_lo, norm_hi};
            fwrite(iv, sizeof iv, 1, stf);
            fwrite(fv, sizeof fv, 1, stf);
            fwrite(st.last_sample_buffer, sizeof(float), FFT_HALF * 9, stf);        // the nine arrays, contiguous in nr_spectral_t's order
        } else if (op != '\n' && op != '#') return 3;
    }
    fclose(outf); fclose(stf); fclose(trf);
    return 0;
}
