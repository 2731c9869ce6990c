// Developer tool (CPU machine only; tools/make_ref_iqd_golden.py builds and runs it): the IQ display extension as the reference runs
// it -- class iq_display (extensions/IQ_display/iq_display.cpp:29-242) over class pll (rx/kiwi/pll.h), as the reference's own
// statements, cut at build time into a temporary directory.  Nothing of the reference's text enters the repository; only the data
// (tests/golden/iqd_ref.npz) does.
//
// What this harness adds (none of the reference's headers is used):
//   * u1_t, TYPECPX, NIQ and CUTESDR_MAX_VAL as types.h / datatypes.h / kiwi.h have them (the tool pins those lines);
//   * ext_send_msg_data() capturing cmd and payload; ext_send_msg() taking the four numbers of the text message off its arguments;
//     adc_clock_system() answering a constant;
//   * what iq_display_msgs (:256-273) does around the class: `N` makes a fresh object (`SET ext_server_init`), `R run rate` is
//     `SET run=%d` -- set_sample_rate(rate) for run != 0 and the registration of the callback: a block reaches display_data only while
//     it is registered.  Every other command goes through process_msg as text.
//
//   iqd_ref script.txt pool.bin out.bin
//       script lines:  N | R run rate | G gain | P points | M pll_mode arg | W bandwidth | D draw | Y display_mode | C
//                      B inst ns off     display_data(inst, ns, pool + off) (pool.bin: complex floats)
//       out.bin: per B int32 rows, per row int32 cmd, int32 len and the bytes; int32 sent and, when sent, float cmaI, cmaQ, double df,
//       float phase, int32 0.  Then the state: int32 points, nsamp, exponent, msk_mode, msk_baud, draw, display_mode, maN, maNsend,
//       ring[2]; float gain, fs, pll_bandwidth, cma.re, cma.im, ama; per PLL (_pll, _pllMinus, _pllPlus) float fs, fc, df, phase, b[0],
//       b[1], ud; _iq, _plot, _map
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <complex>
#include <memory>
#include <vector>

typedef unsigned char u1_t;
struct TYPECPX { float re, im; };
#define NIQ 2
#define CUTESDR_MAX_VAL ((float) ((1 << 15) - 1))
#define IQ_POINTS 0
#define IQ_DENSITY 1
#define N_IQ_RING (16 * 1024)
#define N_CH 2
#define N_HISTORY 2
#define IQ_DISPLAY_DEBUG_MSG false

static double adc_clock_system() { return 66666600.0; }

static std::vector<unsigned char> sent_rows;
static int nrows;
static int ext_send_msg_data(int rx_chan, bool debug, u1_t cmd, u1_t *bytes, int nbytes)
{
    if (rx_chan != 0 || nbytes < 0) { fprintf(stderr, "unexpected ext_send_msg_data\n"); exit(7); }
    const int32_t h[2] = {cmd, nbytes};
    sent_rows.insert(sent_rows.end(), (const unsigned char *) h, (const unsigned char *) h + 8);
    sent_rows.insert(sent_rows.end(), bytes, bytes + nbytes);
    nrows++;
    return 0;
}

static int sent;
static struct { float cmaI, cmaQ; double df; float phase; int32_t reserved; } status;
static int ext_send_msg(int rx_chan, bool debug, const char *fmt, ...)
{
    if (strncmp(fmt, "EXT cmaI=", 9)) return 0;
    va_list ap;
    va_start(ap, fmt);
    status.cmaI = (float) va_arg(ap, double);
    status.cmaQ = (float) va_arg(ap, double);
    status.df = va_arg(ap, double);
    status.phase = (float) va_arg(ap, double);
    status.reserved = 0;
    va_end(ap);
    sent++;
    return 0;
}

#define private public
#define protected public
#include "IQD_CUT_PLL.inc"
#include "IQD_CUT_CLASS.inc"
#undef private
#undef protected

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
    iq_display::sptr q;
    bool registered = false;
    char line[256], cmd[300];
    while (fgets(line, sizeof line, sf)) {
        line[strcspn(line, "\n")] = 0;
        const char op = line[0];
        int a = 0, b = 0;
        cmd[0] = 0;
        if (op == 'N') {
            q = iq_display::make(0);
            registered = false;
        } else if (op == 0 || op == '#') {
        } else if (!q) {
            return 5;
        } else if (op == 'R') {
            double rate;
            if (sscanf(line + 1, "%d %lf", &a, &rate) != 2) return 3;
            if (a) q->set_sample_rate(rate);
            registered = a != 0;
        } else if (op == 'G') {
            snprintf(cmd, sizeof cmd, "SET gain=%s", line + 2);
        } else if (op == 'P') {
            snprintf(cmd, sizeof cmd, "SET points=%s", line + 2);
        } else if (op == 'M') {
            if (sscanf(line + 1, "%d %d", &a, &b) != 2) return 3;
            snprintf(cmd, sizeof cmd, "SET pll_mode=%d arg=%d", a, b);
        } else if (op == 'W') {
            snprintf(cmd, sizeof cmd, "SET pll_bandwidth=%s", line + 2);
        } else if (op == 'D') {
            snprintf(cmd, sizeof cmd, "SET draw=%s", line + 2);
        } else if (op == 'Y') {
            snprintf(cmd, sizeof cmd, "SET display_mode=%s", line + 2);
        } else if (op == 'C') {
            snprintf(cmd, sizeof cmd, "SET clear");
        } else if (op == 'B') {
            int inst, ns;
            unsigned long off;
            if (sscanf(line + 1, "%d %d %lu", &inst, &ns, &off) != 3 || ns < 1 || off + ns > npool) return 3;
            sent_rows.clear();
            nrows = 0;
            sent = 0;
            if (registered) q->display_data(inst, ns, (TYPECPX *) pool.data() + off);
            fwrite(&nrows, 4, 1, of);
            if (!sent_rows.empty()) fwrite(sent_rows.data(), 1, sent_rows.size(), of);
            fwrite(&sent, 4, 1, of);
            if (sent) fwrite(&status, sizeof status, 1, of);
        } else return 3;
        if (cmd[0]) q->process_msg(cmd);
    }
    if (!q) return 5;
    const int32_t iv[11] = {q->_points, q->_nsamp, q->_exponent, q->_msk_mode ? 1 : 0, q->_msk_baud, q->_draw, q->_display_mode, q->_maN, q->_maNsend,
                            q->_ring[0], q->_ring[1]};
    const float fv[6] = {q->_gain, q->_fs, q->_pll_bandwidth, q->_cma.real(), q->_cma.imag(), q->_ama};
    fwrite(iv, sizeof iv, 1, of);
    fwrite(fv, sizeof fv, 1, of);
    pll *plls[3] = {&q->_pll, &q->_pllMinus, &q->_pllPlus};
    for (int w = 0; w < 3; w++) {
        const pll &p = *plls[w];
        const float pv[7] = {p._fs, p._fc, p._df, p._phase, p._b[0], p._b[1], p._ud};
        fwrite(pv, sizeof pv, 1, of);
    }
    fwrite(q->_iq, sizeof q->_iq, 1, of);
    fwrite(q->_plot, sizeof q->_plot, 1, of);
    fwrite(q->_map, sizeof q->_map, 1, of);
    fclose(of);
    return 0;
}
