// What tools/ref/ref_wspr_main.cpp (the reference's own statements, cut at build time) and tools/wspr_host_driver.cpp (csrc/kg_wspr.h on
// the host) share, all of it ours: the stand-in for FFTW, the records of out.bin and the script loop.  Each harness defines the hooks
// h_init .. h_dump ahead of including this file.
//
//   <exe> script.txt pool.bin out.bin planes.bin
//       script lines:  I snd_rate          `SET ext_server_init`; int_decimate = (int) (snd_rate / 375.0)
//                      C 0|1               `SET capture=`
//                      Y 2|15              wspr_type
//                      M 0|1               more_candidates
//                      B off n min sec     one callback of wspr_data: n complex samples at complex offset off of pool.bin (float32 pairs), at min:sec
//                      L file              pwr_samp [512][348] then pwr_sampavg [512] (float32) into half 0, then pass 0 of wspr_decode on it
//       out.bin, int32 words:  1 blk status                               a status change (blk -1: by a command)
//                              4 blk group half savg[512]                 ahead of every row
//                              2 blk group half tsync bytes[412 as 103 words]
//                              3 blk half npk pk[12][3] cand[12][6] cond[4]   a cycle end; cond: what the harness adds (zeros where it adds nothing)
//                              5 info[18]                                 the end state (kg_wspr_info without snd_rate)
//       planes.bin: pwr_sampavg [2][512], pwr_samp [2][512][348], i_data [2][45000], q_data [2][45000]
// FFTW is not on this machine.  wspr_dft512 evaluates the 512-point forward DFT in double and rounds to float; with -DWSPR_DFT_FP32 it
// is an independent radix-2 transform in float: the pair measures what two correct transforms differ by in the rows.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

static void wspr_dft512(const float (*in)[2], float (*out)[2])
{
    enum { N = 512 };
#ifdef WSPR_DFT_FP32
    static float wr[N / 2], wi[N / 2];
    static bool init;
    if (!init) {
        for (int k = 0; k < N / 2; k++) { wr[k] = (float) cos(2 * M_PI * k / N); wi[k] = (float) -sin(2 * M_PI * k / N); }
        init = true;
    }
    float re[N], im[N];
    for (int n = 0; n < N; n++) {
        int r = 0;
        for (int b = 0; b < 9; b++) r |= ((n >> b) & 1) << (8 - b);
        re[r] = in[n][0]; im[r] = in[n][1];
    }
    for (int len = 2; len <= N; len <<= 1)
        for (int s = 0; s < N; s += len)
            for (int k = 0; k < len / 2; k++) {
                const float c = wr[k * (N / len)], d = wi[k * (N / len)];
                const int a = s + k, b = a + len / 2;
                const float tr = re[b] * c - im[b] * d, ti = re[b] * d + im[b] * c;
                re[b] = re[a] - tr; im[b] = im[a] - ti;
                re[a] = re[a] + tr; im[a] = im[a] + ti;
            }
    for (int k = 0; k < N; k++) { out[k][0] = re[k]; out[k][1] = im[k]; }
#else
    static double c[N], s[N];
    static bool init;
    if (!init) {
        for (int k = 0; k < N; k++) { c[k] = (double) cosl(2 * M_PIl * k / N); s[k] = (double) sinl(2 * M_PIl * k / N); }
        init = true;
    }
    for (int k = 0; k < N; k++) {
        double re = 0, im = 0;
        for (int n = 0; n < N; n++) {
            const int t = (n * k) & (N - 1);
            re += (double) in[n][0] * c[t] + (double) in[n][1] * s[t];
            im += (double) in[n][1] * c[t] - (double) in[n][0] * s[t];
        }
        out[k][0] = (float) re; out[k][1] = (float) im;
    }
#endif
}

static std::vector<int32_t> g_out;
static int g_blk = -1;
static int32_t bits_of(float f) { int32_t i; memcpy(&i, &f, 4); return i; }
static void rec_status(int status) { g_out.push_back(1); g_out.push_back(g_blk); g_out.push_back(status); }
static void rec_row(int group, int half, const float *savg, const unsigned char *ws)
{
    g_out.push_back(4); g_out.push_back(g_blk); g_out.push_back(group); g_out.push_back(half);
    for (int j = 0; j < 512; j++) g_out.push_back(bits_of(savg[j]));
    g_out.push_back(2); g_out.push_back(g_blk); g_out.push_back(group); g_out.push_back(half); g_out.push_back(ws[0]);
    int32_t w[103];
    memcpy(w, ws, 412);
    g_out.insert(g_out.end(), w, w + 103);
}
struct rec_pk { int bin0; float freq0, snr0; };
struct rec_cand { float freq0; int shift0; float drift0, sync0; int freq_idx, bin0; };
static void rec_cycle(int half, int npk, const rec_pk *pk, const rec_cand *cand, const int32_t *cond)
{
    g_out.push_back(3); g_out.push_back(g_blk); g_out.push_back(half); g_out.push_back(npk);
    for (int r = 0; r < 12; r++) {
        const rec_pk z = {0, 0, 0};
        const rec_pk &p = r < npk ? pk[r] : z;
        g_out.push_back(p.bin0); g_out.push_back(bits_of(p.freq0)); g_out.push_back(bits_of(p.snr0));
    }
    for (int r = 0; r < 12; r++) {
        const rec_cand z = {0, 0, 0, 0, 0, 0};
        const rec_cand &c = r < npk ? cand[r] : z;
        g_out.push_back(bits_of(c.freq0)); g_out.push_back(c.shift0); g_out.push_back(bits_of(c.drift0)); g_out.push_back(bits_of(c.sync0));
        g_out.push_back(c.freq_idx); g_out.push_back(c.bin0);
    }
    for (int r = 0; r < 4; r++) g_out.push_back(cond ? cond[r] : 0);
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

// the hooks; a refusal is a status 11 .. 14 (rate, type, time, not initialised)
static int h_init(double snd_rate);
static int h_capture(int on);
static int h_type(int type);
static int h_more(int on);
static int h_block(const float *iq, int n, int min, int sec);
static int h_load(const float *pwr_samp, const float *pwr_sampavg);
static void h_dump(int32_t *info18, FILE *planes);

int main(int argc, char **argv)
{
    if (argc != 5) { fprintf(stderr, "usage: %s script.txt pool.bin out.bin planes.bin\n", argv[0]); return 2; }
    FILE *sf = fopen(argv[1], "r"), *of = fopen(argv[3], "wb"), *pf = fopen(argv[4], "wb");
    if (!sf || !of || !pf) return 2;
    std::vector<unsigned char> pool = slurp(argv[2]);
    const size_t npool = pool.size() / (2 * sizeof(float));
    char line[512];
    int nblk = 0;
    while (fgets(line, sizeof line, sf)) {
        line[strcspn(line, "\n")] = 0;
        const char op = line[0];
        int a, rc = 0;
        double r;
        g_blk = -1;
        if (op == 0 || op == '#') {
        } else if (op == 'I') {
            if (sscanf(line + 1, "%lf", &r) != 1) return 3;
            rc = h_init(r);
        } else if (op == 'C') {
            if (sscanf(line + 1, "%d", &a) != 1) return 3;
            rc = h_capture(a);
        } else if (op == 'Y') {
            if (sscanf(line + 1, "%d", &a) != 1) return 3;
            rc = h_type(a);
        } else if (op == 'M') {
            if (sscanf(line + 1, "%d", &a) != 1) return 3;
            rc = h_more(a);
        } else if (op == 'B') {
            unsigned long off;
            int n, min, sec;
            if (sscanf(line + 1, "%lu %d %d %d", &off, &n, &min, &sec) != 4 || n < 1 || off + (unsigned long) n > npool) return 3;
            g_blk = nblk++;
            rc = h_block((const float *) pool.data() + 2 * off, n, min, sec);
        } else if (op == 'L') {
            std::vector<unsigned char> pl = slurp(line + 2);
            if (pl.size() != sizeof(float) * (512 * 348 + 512)) return 3;
            g_blk = nblk++;
            rc = h_load((const float *) pl.data(), (const float *) pl.data() + 512 * 348);
        } else return 3;
        if (rc) return rc;
    }
    int32_t info[18];
    h_dump(info, pf);
    g_out.push_back(5);
    g_out.insert(g_out.end(), info, info + 18);
    fwrite(g_out.data(), 4, g_out.size(), of);
    fclose(of); fclose(pf);
    return 0;
}
