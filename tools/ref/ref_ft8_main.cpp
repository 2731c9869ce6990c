// The harness tools/make_ref_ft8_golden.py compiles around statements cut from the reference at run time (each FT8_CUT_* is a file the
// maker writes into its temporary directory; the reference's headers and its kiss_fft / constants sources are read in place from the
// reference tree).  Stubs of ours stand where the server would: the clock is the scene's, decode() ends at log174, nothing is sent.
// With -DFT8_DFT_DOUBLE monitor_process calls the independent double-precision DFT of ft8_harness.h in kiss_fftr's place (build B).
#include <stdarg.h>
#include <time.h>

#include "ft8_harness.h"

extern "C" {
#include <ft8/constants.h>
#include <ft8/decode.h>
#include <common/monitor.h>
}

typedef uint32_t u4_t;
typedef uint8_t u1_t;
typedef int16_t s2_t;
typedef float TYPEREAL;
typedef int16_t TYPEMONO16;
#define MAX_RX_CHANS 1
#include FT8_CUT_PASSBAND
#define LOG(...)
#define NextTask(s)
static double snd_rate = 12000;
static struct { float SNR_adj; } ft8_conf = {H_SNR_ADJ};
static void hashtable_init(int) {}
static void PSKReporter_reset(int) {}
static void ext_send_msg_encoded(int, bool, const char *, const char *, const char *, ...) {}

static double g_now;                                        // the scene's clock reading of the callback under way
static int ref_clock_gettime(int, struct timespec *ts)
{
    ts->tv_sec = (time_t) floor(g_now);
    ts->tv_nsec = (long) llround((g_now - floor(g_now)) * 1e9);
    return 0;
}
#define clock_gettime(id, ts) ref_clock_gettime(id, ts)

#ifdef FT8_DFT_DOUBLE
#define kiss_fftr(cfg, in, out) h_dft_double(me->nfft, in, (float *) (out), me->min_bin * me->wf.freq_osr, me->max_bin * me->wf.freq_osr)
#endif

// common/monitor.c
#include FT8_CUT_HANN
#include FT8_CUT_WFALL
#include FT8_CUT_MON
// ft8/decode.c
#include FT8_CUT_CANDMAG
#include FT8_CUT_MAX
#include FT8_CUT_HEAPS
#include FT8_CUT_SYM4
#include FT8_CUT_SYM8
#include FT8_CUT_SCORE
#include FT8_CUT_FIND
#include FT8_CUT_LIKE
// ft8_lib/decode_ft8.c
#include FT8_CUT_STRUCT
#include FT8_CUT_ARRAY
#include FT8_CUT_CONSTS

static int g_cb;
static uint32_t g_slot_seen;
static void flush_start()
{
    decode_ft8_t *ft8 = &decode_ft8[0];
    if (ft8->slot != g_slot_seen) {
        g_slot_seen = ft8->slot;
        h_event(g_cb, 0, (int) ft8->slot, (int) ft8->decode_time, (int64_t) timegm(&ft8->tm_slot_start));
    }
}
static void record_slot(const monitor_t *mon, int num_candidates, int min_score)
{
    const ftx_waterfall_t *wf = &mon->wf;
    ftx_candidate_t candidate_list[kMax_candidates];
    const int n = ftx_find_candidates(wf, num_candidates, candidate_list, min_score);
    std::vector<h_cand> hc((size_t) n);
    std::vector<float> logs((size_t) n * FTX_LDPC_N);
    for (int idx = 0; idx < n; ++idx) {
        const ftx_candidate_t *cand = &candidate_list[idx];
#include FT8_CUT_FREQ
#include FT8_CUT_SNR
        hc[idx] = h_cand{cand->score, cand->time_offset, cand->freq_offset, cand->time_sub, cand->freq_sub, freq_hz, time_sec, snr};
        {
#include FT8_CUT_L174
            memcpy(&logs[(size_t) idx * FTX_LDPC_N], log174, sizeof log174);
        }
    }
    h_slot(g_cb, wf->num_blocks, n, mon->max_mag, hc.data(), logs.data(), wf->mag, (size_t) wf->num_blocks * wf->block_stride);
}
static void decode(int rx_chan, const monitor_t *mon, int freqHz)
{
    decode_ft8_t *ft8 = &decode_ft8[rx_chan];
    flush_start();
    h_event(g_cb, 1, mon->wf.num_blocks, (int) ft8->slot, (int64_t) timegm(&ft8->tm_slot_start));
    record_slot(mon, kMax_candidates, kMin_score);
}

#include FT8_CUT_SAMPLES
#include FT8_CUT_INIT

int main(int argc, char **argv)
{
    if (argc != 3) return 1;
    h_scene s;
    if (h_read_scene(argv[1], s)) return 2;
    h_out = fopen(argv[2], "wb");
    if (!h_out) return 3;
    decode_ft8_t *ft8 = &decode_ft8[0];
    decode_ft8_protocol(0, 0, s.hd[1]);
    monitor_t *mon = &ft8->mon;
    h_sizes(mon->block_size, mon->nfft, mon->wf.num_bins, mon->min_bin, mon->wf.max_blocks, ft8->num_samples, mon->wf.block_stride, mon->subblock_size, mon->window);
    if (s.hd[0] == H_LOAD) {
        if (s.hd[2] < 1 || s.hd[2] > mon->wf.max_blocks || s.mag.size() != (size_t) s.hd[2] * mon->wf.block_stride) return 4;
        memcpy(mon->wf.mag, s.mag.data(), s.mag.size());
        mon->wf.num_blocks = s.hd[2];
        record_slot(mon, s.hd[3], s.hd[4]);
    } else {
        const int ns = s.hd[2];
        u1_t start_test = 0;
        for (int cb = 0; cb < s.hd[3]; cb++) {
            if (cb == s.hd[4]) { decode_ft8_protocol(0, 0, s.hd[5]); g_slot_seen = 0; }
            g_now = s.times[cb];
            g_cb = cb;
            decode_ft8_samples(0, &s.samples[(size_t) cb * ns], ns, 0, &start_test);
            flush_start();
        }
        h_end(ft8->tsync, ft8->in_pos, ft8->frame_pos, mon->wf.num_blocks, ft8->slot, ft8->decode_time, mon->nfft, mon->max_mag, mon->last_frame, mon->wf.mag,
              (size_t) mon->wf.num_blocks * mon->wf.block_stride);
    }
    fclose(h_out);
    return 0;
}
