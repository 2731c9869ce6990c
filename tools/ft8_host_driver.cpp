// csrc/kg_ft8.h on the host: the twin the FT8 / FT4 kernels are held to, behind the scene and records of tools/ref/ft8_harness.h, so that
// tests/test_ft8_cpu.py can compare it with tests/golden/ft8_ref.npz (made from the reference's own statements) record by record.
// The schedule is kg_ft8.h's sched_callback, the ops are carried out as the kernels do -- two sample buffers by slot parity, the tail
// handed over at a slot's end -- with the transform of the build: h_dft_double (the golden's build B), or with -DFT8_USE_KISS the
// reference's kiss_fftr, linked in by the golden's maker alone (build A).  With the same transform every byte, max_mag, candidate and
// log174 is the reference's bit for bit.  Built with g++ -O2 -ffp-contract=off.
#include "../flydog_sdr_gps_amd/csrc/kg_ft8.h"

using namespace kg_ft8_cf;

#include "ref/ft8_harness.h"

#ifdef FT8_USE_KISS
extern "C" {
#include <fft/kiss_fftr.h>
}
#endif

enum { SLOT_SAMPLES = 92 * 1920 + MAX_NS, WF_BYTES = 93 * 4 * 481 };
static state_t st;
static std::vector<float> buf[2], win;
static std::vector<uint8_t> wf[2];
static float max_mag;

static void transform(const cfg_t &c, const float *timedata, float *freq)
{
#ifdef FT8_USE_KISS
    static kiss_fftr_cfg cfg;
    static int have;
    if (have != c.nfft) { cfg = kiss_fftr_alloc(c.nfft, 0, 0, 0); have = c.nfft; }
    kiss_fftr(cfg, timedata, (kiss_fft_cpx *) freq);
#else
    h_dft_double(c.nfft, timedata, freq, c.min_bin * FREQ_OSR, c.max_bin * FREQ_OSR);
#endif
}

static void do_block(const cfg_t &c, int parity, int block, int frame_pos)
{
    std::vector<float> timedata((size_t) c.nfft), freq((size_t) c.nfft + 2);
    const float *slot0 = buf[parity].data() + MAX_NFFT;
    for (int t = 0; t < TIME_OSR; t++) {
        const float *x = slot0 + frame_start(c, frame_pos, t);
        for (int pos = 0; pos < c.nfft; pos++) timedata[pos] = windowed(win[pos], x[pos]);
        transform(c, timedata.data(), freq.data());
        for (int freq_sub = 0; freq_sub < FREQ_OSR; freq_sub++)
            for (int bin = 0; bin < c.num_bins; bin++) {
                const int k = src_bin_of(c.min_bin, bin, freq_sub);
                const float db = db_of(freq[2 * k], freq[2 * k + 1]);
                wf[parity][mag_index(c, block, t, freq_sub, bin)] = byte_of(db);
                if (db > max_mag) max_mag = db;
            }
    }
}

static void do_slot(const cfg_t &c, const uint8_t *mag, int cb, int num_blocks, int num_candidates, int min_score, float mm)
{
    static slot_t sl;
    slot_end(c, mag, num_blocks, num_candidates, min_score, H_SNR_ADJ, sl);
    std::vector<h_cand> hc((size_t) sl.ncand);
    for (int i = 0; i < sl.ncand; i++)
        hc[i] = h_cand{sl.cand[i].score, sl.cand[i].time_offset, sl.cand[i].freq_offset, sl.cand[i].time_sub, sl.cand[i].freq_sub, sl.freq_hz[i], sl.time_sec[i], sl.snr[i]};
    h_slot(cb, num_blocks, sl.ncand, mm, hc.data(), &sl.log174[0][0], mag, (size_t) num_blocks * c.block_stride);
}

static int h_init(int protocol)
{
    if (cmd_init(st, protocol, 12000.0)) return 11;
    win.resize((size_t) st.cfg.nfft);
    for (int i = 0; i < st.cfg.nfft; i++) win[i] = window_at(st.cfg, i);
    for (int p = 0; p < 2; p++) { buf[p].assign((size_t) MAX_NFFT + SLOT_SAMPLES, 0.0f); wf[p].assign(WF_BYTES, 0); }
    max_mag = -120.0f;
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 1;
    h_scene s;
    if (h_read_scene(argv[1], s)) return 2;
    h_out = fopen(argv[2], "wb");
    if (!h_out) return 3;
    if (int rc = h_init(s.hd[1])) return rc;
    const cfg_t c0 = st.cfg;
    h_sizes(c0.block_size, c0.nfft, c0.num_bins, c0.min_bin, c0.max_blocks, c0.num_samples, c0.block_stride, c0.subblock_size, win.data());
    if (s.hd[0] == H_LOAD) {
        if (s.hd[2] < 1 || s.hd[2] > c0.max_blocks || s.mag.size() != (size_t) s.hd[2] * c0.block_stride) return 4;
        if (s.hd[3] < 1 || s.hd[3] > MAX_CAND) return 5;
        do_slot(c0, s.mag.data(), 0, s.hd[2], s.hd[3], s.hd[4], -120.0f);
    } else {
        const int ns = s.hd[2];
        if (ns < 1 || ns > MAX_NS) return 6;
        for (int cb = 0; cb < s.hd[3]; cb++) {
            if (cb == s.hd[4])
                if (int rc = h_init(s.hd[5])) return rc;
            if (!time_ok(s.times[cb])) return 13;
            const cfg_t c = st.cfg;
            sched_t sp;
            sched_callback(st, sp, cb, 0, ns, s.times[cb]);
            if (sp.nend > 1) return 20;
            for (const ev_t &m : sp.evs)
                if (m.kind == EV_SLOT_START) h_event(cb, m.kind, m.a, m.b, m.t);
            for (const op_t &o : sp.ops) {
                if (o.kind == OP_COPY)
                    for (int t = 0; t < o.n; t++) buf[o.parity][(size_t) MAX_NFFT + o.a + t] = sample_of(s.samples[(size_t) cb * ns + o.src + t]);
                else if (o.kind == OP_BLOCK) do_block(c, o.parity, o.a, (int) o.src);
                else {
#ifdef KG_FT8_MUT_TAIL                                       /* tests/test_ft8_cpu.py: the golden must notice a last_frame that does not survive the slot */
                    memset(&buf[o.parity ^ 1][MAX_NFFT - c.nfft], 0, sizeof(float) * c.nfft);
#else
                    memcpy(&buf[o.parity ^ 1][MAX_NFFT - c.nfft], &buf[o.parity][(size_t) MAX_NFFT + o.a * c.block_size - c.nfft], sizeof(float) * c.nfft);
#endif
                    for (const ev_t &m : sp.evs)
                        if (m.kind == EV_DECODE) h_event(cb, m.kind, m.a, m.b, m.t);
                    do_slot(c, wf[o.parity].data(), cb, o.a, MAX_CAND, MIN_SCORE, max_mag);
                    max_mag = -120.0f;                                  // monitor_reset
                }
            }
        }
        const cfg_t &c = st.cfg;
        const float *lf = &buf[st.parity][(size_t) MAX_NFFT - c.nfft + (st.tsync ? st.frame_pos : 0)];
        h_end(st.tsync, st.in_pos, st.frame_pos, st.num_blocks, st.slot, st.decode_time, c.nfft, max_mag, lf, wf[st.parity].data(), (size_t) st.num_blocks * c.block_stride);
    }
    fclose(h_out);
    return 0;
}
