// csrc/kg_wspr_dec.h on the host: the twin the stage-2 WSPR kernels are held to, behind the scene files of tools/ref/ref_wspr_dec_main.cpp,
// so that tests/test_wspr_dec_cpu.py and tools/make_ref_wspr_dec_golden.py can compare it with the reference record by record.
// Built with g++ -O2 -ffp-contract=off (a test adds -DKG_WSPR_DEC_MUT_* to see that the golden notices).
//   driver scene out jig mettab watch     the passes of a scene: records, every jiggle's bytes; watch: float least margin, int32 strict,
//                                         float least distance of a pre-clamp soft value from an integer, per pass
//   driver -f symbols n maxcycles mettab out     fano alone on n deinterleaved sets: per set int32 ok, uint32 metric, cycles, maxnp, 10 bytes + 2 pad
// Refusals (exit status): 11 no table, 12 a candidate out of range, 13 iifac, 14 maxcycles -- as kg_wspr_decode / kg_wspr_load_iq refuse.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../flydog_sdr_gps_amd/csrc/kg_wspr_dec.h"

using namespace kg_wspr_df;

static bool read_table(const char *path, int32_t *mettab)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    const bool ok = fread(mettab, 4, 512, f) == 512;
    fclose(f);
    for (int i = 0; ok && i < 512; i++)
        if (mettab[i] > MAX_METRIC || mettab[i] < -MAX_METRIC) return false;
    return ok;
}

int main(int argc, char **argv)
{
    static int32_t mettab[512];
    if (argc == 7 && !strcmp(argv[1], "-f")) {
        const int n = atoi(argv[3]);
        const long mc = atol(argv[4]);
        if (!read_table(argv[5], mettab)) return 11;
        if (mc < 1 || mc > MAX_MAXCYCLES) return 14;
        std::vector<uint8_t> sy((size_t) n * NSYM);
        FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[6], "wb");
        if (!in || !out || fread(sy.data(), NSYM, n, in) != (size_t) n) return 4;
        for (int s = 0; s < n; s++) {
            struct { int32_t ok; uint32_t metric, cycles, maxnp; uint8_t data[12]; } o;
            memset(&o, 0, sizeof o);
            o.ok = fano_host(sy.data() + (size_t) s * NSYM, mettab, (uint32_t) mc, &o.metric, &o.cycles, &o.maxnp, o.data);
            fwrite(&o, sizeof o, 1, out);
        }
        fclose(out);
        return 0;
    }
    if (argc != 6) { fprintf(stderr, "usage: %s scene out jig mettab watch | -f symbols n maxcycles mettab out\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 3;
    if (!read_table(argv[4], mettab)) return 11;
    FILE *out = fopen(argv[2], "wb"), *jig = fopen(argv[3], "wb"), *wf = fopen(argv[5], "wb");
    if (!out || !jig || !wf) return 3;
    int32_t head[2];
    if (fread(head, 4, 2, in) != 2 || head[0] < 0 || head[0] > kg_wspr_cf::MAX_NPK) return 4;
    static float idat[TPOINTS], qdat[TPOINTS];
    if (fread(idat, 4, TPOINTS, in) != TPOINTS || fread(qdat, 4, TPOINTS, in) != TPOINTS) return 4;
    struct cd_t { float freq0; int32_t shift0; float drift0, sync0; } cd[kg_wspr_cf::MAX_NPK];
    int32_t ignore[kg_wspr_cf::MAX_NPK] = {0};
    for (int c = 0; c < head[0]; c++) {
        if (fread(&cd[c], sizeof(cd_t), 1, in) != 1) return 4;
        if (!(fabsf(cd[c].freq0) <= 113) || abs(cd[c].shift0) > TPOINTS || !(fabsf(cd[c].drift0) <= 4)) return 12;
    }
    static uint8_t w_symbols[NSYM];
    static watch_t watch;
    for (int ps = 0; ps < head[1]; ps++) {
        int32_t a[3];
        if (fread(a, 4, 3, in) != 3) return 4;
        if (a[1] < 1 || a[1] > JIG_RANGE) return 13;
        if (a[0] < 1 || a[0] > MAX_MAXCYCLES) return 14;
        margin_t mg = {INFINITY, 1};
        float int_dist = INFINITY;
        for (int c = 0; c < head[0]; c++) {
            rec_t r;
            memset(&watch, 0, sizeof watch);
            watch.mg = mg;
            watch.int_dist = int_dist;
            decode_candidate(idat, qdat, mettab, cd[c].freq0, cd[c].shift0, cd[c].drift0, cd[c].sync0, &ignore[c], (uint32_t) a[0], a[1], a[2], w_symbols, r, &watch);
            mg = watch.mg;
            int_dist = watch.int_dist;
            fwrite(&r, sizeof r, 1, out);
            fwrite(watch.jig_syms, NSYM, watch.njig, jig);
        }
        fwrite(&mg.least, 4, 1, wf);
        fwrite(&mg.strict, 4, 1, wf);
        fwrite(&int_dist, 4, 1, wf);
    }
    fclose(out); fclose(jig); fclose(wf);
    return 0;
}
