// Developer tool (CPU machine only; tools/make_ref_lorc_golden.py builds and runs it): the Loran-C extension as the reference runs it
// -- the structs (extensions/Loran_C/loran_c.cpp:29-52), loran_c_data (:65-196) and init_gri (:198-208) as the reference's own
// statements, cut at build time into a temporary directory.  Nothing of the reference's text enters the repository; only the data
// (tests/golden/lorc_ref.npz) does.
//
// What this harness adds (none of the reference's headers is used):
//   * u1_t, u4_t, TYPECPX, CUTESDR_MAX_VAL, MAX_RX_CHANS and the extension's own constants as the pinned lines have them;
//   * ext_send_msg_data() recording the row with the sample it went out at (the channel's samp counter less what it was when the
//     block began); panic();
//   * the commands of loran_c_msgs (:218-302), restated from the pinned lines: `N srate i_srate` is `SET ext_server_init` (the memset;
//     srate is what ext_update_get_sample_rateHz answers, i_srate is snd_rate), `S` / `T` register and unregister the callback: a block
//     reaches loran_c_data only while it is registered.
//
//   lorc_ref script.txt pool.bin out.bin
//       script lines:  N srate i_srate | I ch gri | O ch offset | G ch gain | A ch avg_algo | P ch avg_param | S | T
//                      B ns off     loran_c_data(0, 0, ns, pool + off) (pool.bin: complex floats)
//       out.bin: per B int32 rows, per row int32 samp, ch, cmd, len and the bytes.  Then the state: int32 i_srate, redraw_legend, double
//       srate; per channel u4 gri, samp, nbucket, dsp_samps, avg_samps, navgs, double samp_per_GRI, float gain, max, int32 offset,
//       avg_algo, double avg_param_f, int32 avg_param_i, restart; avg[2][1199]
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <unistd.h>

#include <vector>

typedef unsigned int u4_t;
typedef unsigned char u1_t;
struct TYPECPX { float re, im; };
#define CUTESDR_MAX_VAL ((float) ((1 << 15) - 1))
#define MAX_RX_CHANS 16
#define LORAN_C_DEBUG_MSG false
#define SCOPE_DATA 0
#define SCOPE_RESET 1
#define GRI_2_SEC(gri) ((double) (gri) / 1e5)
#define SND_RATE_HALF_THRESHOLD 12000
#define MAX_GRI 9999
#define MAX_BUCKET (int) (SND_RATE_HALF_THRESHOLD * GRI_2_SEC(MAX_GRI))
#define AVG_CMA 0
#define AVG_EMA 1
#define AVG_IIR 2
#define USE_IQ

static void panic(const char *why) { fprintf(stderr, "panic: %s\n", why); exit(8); }

#include "LORC_CUT_STRUCTS.inc"

static loran_c_t loran_c[MAX_RX_CHANS];
static u4_t samp0[2];
static std::vector<unsigned char> sent_rows;
static int nrows;
static int ext_send_msg_data(int rx_chan, bool debug, u1_t cmd, u1_t *bytes, int nbytes)
{
    if (rx_chan != 0 || nbytes < 1 || bytes[0] > 1) { fprintf(stderr, "unexpected ext_send_msg_data\n"); exit(7); }
    const int ch = bytes[0];
    const int32_t h[4] = {(int32_t) (loran_c[0].ch[ch].samp - samp0[ch]), ch, cmd, nbytes};
    sent_rows.insert(sent_rows.end(), (const unsigned char *) h, (const unsigned char *) h + 16);
    sent_rows.insert(sent_rows.end(), bytes, bytes + nbytes);
    nrows++;
    return 0;
}

#include "LORC_CUT_DATA.inc"
#include "LORC_CUT_GRI.inc"

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
    if (argc != 4) { fprintf(stderr, "usage: %s script.txt pool.bin out.bin\n", argv[0]); return 2; }
    FILE *sf = fopen(argv[1], "r"), *of = fopen(argv[3], "wb");
    if (!sf || !of) return 2;
    std::vector<unsigned char> pool = slurp(argv[2]);
    const size_t npool = pool.size() / sizeof(TYPECPX);
    loran_c_t *e = &loran_c[0];
    loran_c_ch_t *c;
    bool registered = false, inited = false;
    char line[256];
    while (fgets(line, sizeof line, sf)) {
        line[strcspn(line, "\n")] = 0;
        const char op = line[0];
        int ch = 0, a = 0;
        double v;
        if (op == 'N') {
            if (sscanf(line + 1, "%lf %d", &v, &a) != 2) return 3;
            memset(e, 0, sizeof(loran_c_t));
            e->rx_chan = 0;
            e->srate = v;
            e->i_srate = a;
            inited = true;
        } else if (op == 0 || op == '#') {
        } else if (!inited) {
            return 5;
        } else if (op == 'I') {
            if (sscanf(line + 1, "%d %d", &ch, &a) != 2 || ch < 0 || ch > 1) return 3;
            c = &(e->ch[ch]);
            init_gri(e, ch, a);
            e->redraw_legend = true;
            c->restart = true;
        } else if (op == 'O') {
            if (sscanf(line + 1, "%d %d", &ch, &a) != 2 || ch < 0 || ch > 1) return 3;
            const int offset = a;
            c = &(e->ch[ch]);
            c->offset = (c->offset + offset) % c->nbucket;
            c->restart = true;
        } else if (op == 'G') {
            if (sscanf(line + 1, "%d %d", &ch, &a) != 2 || ch < 0 || ch > 1) return 3;
            const int gain = a;
            c = &(e->ch[ch]);
            c->gain = gain? pow(10.0, ((float) -gain) / 10.0) : 0;
            c->restart = true;
        } else if (op == 'A') {
            if (sscanf(line + 1, "%d %d", &ch, &a) != 2 || ch < 0 || ch > 1) return 3;
            c = &(e->ch[ch]);
            c->avg_algo = a;
            c->restart = true;
        } else if (op == 'P') {
            if (sscanf(line + 1, "%d %lf", &ch, &v) != 2 || ch < 0 || ch > 1) return 3;
            const double avg_param = v;
            c = &(e->ch[ch]);
            c->avg_param_f = avg_param;
            c->avg_param_i = lround(avg_param);
            c->restart = true;
        } else if (op == 'S') {
            e->redraw_legend = true;
            e->ch[0].restart = e->ch[1].restart = true;
            registered = true;
        } else if (op == 'T') {
            registered = false;
        } else if (op == 'B') {
            int ns;
            unsigned long off;
            if (sscanf(line + 1, "%d %lu", &ns, &off) != 2 || ns < 1 || off + ns > npool) return 3;
            sent_rows.clear();
            nrows = 0;
            samp0[0] = e->ch[0].samp; samp0[1] = e->ch[1].samp;
            if (registered) loran_c_data(0, 0, ns, (TYPECPX *) pool.data() + off);
            fwrite(&nrows, 4, 1, of);
            if (!sent_rows.empty()) fwrite(sent_rows.data(), 1, sent_rows.size(), of);
        } else return 3;
    }
    if (!inited) return 5;
    const int32_t head[2] = {(int32_t) e->i_srate, e->redraw_legend ? 1 : 0};
    fwrite(head, sizeof head, 1, of);
    fwrite(&e->srate, 8, 1, of);
    for (int k = 0; k < 2; k++) {
        c = &(e->ch[k]);
        const u4_t u[6] = {c->gri, c->samp, c->nbucket, c->dsp_samps, c->avg_samps, c->navgs};
        const float f[2] = {c->gain, c->max};
        const int32_t i1[2] = {c->offset, c->avg_algo}, i2[2] = {c->avg_param_i, c->restart ? 1 : 0};
        fwrite(u, sizeof u, 1, of); fwrite(&c->samp_per_GRI, 8, 1, of); fwrite(f, sizeof f, 1, of); fwrite(i1, sizeof i1, 1, of);
        fwrite(&c->avg_param_f, 8, 1, of); fwrite(i2, sizeof i2, 1, of);
    }
    for (int k = 0; k < 2; k++) fwrite(e->ch[k].avg, sizeof e->ch[k].avg, 1, of);
    fclose(of);
    return 0;
}
