// kg_ft8.h -- the FT8 / FT4 extension (extensions/FT8/, ft8_lib), stage 1: from the real-samples tap to log174, the normalised soft
// bits of every candidate.  On the device AND the host, in the reference's own operand types; library, host driver and golden are built
// with -ffp-contract=off.  What lives here:
//   * decode_ft8_samples and decode_ft8_init / _free / _protocol (ft8_lib/decode_ft8.c:503-620): the sync to the slot, in_pos and
//     frame_pos, which blocks are due, when the slot ends.  NO SAMPLE DRIVES ANY OF IT: sched_callback() walks one callback on sample
//     counts and on the clock the caller hands in and emits the copy run, the blocks due and the events as records;
//   * monitor_init / _process / _reset (common/monitor.c:55-203, WF_ELEM_T uint8_t): the sizes, the window, the analysis frame, the
//     chain mag2 -> dB -> byte, max_mag.  The transform itself is the caller's (the reference links kiss_fftr);
//   * ft8_sync_score, ft4_sync_score, ftx_find_candidates, heapify_up / _down (ft8/decode.c:63-254, :403-454);
//   * ft8 / ft4_extract_likelihood, _extract_symbol, ftx_normalize_logl (:256-328, :457-485);
//   * freq_hz, time_sec and snr of a candidate (decode_ft8.c:229-230, :303) with SNR_adj as an input.
// Kept to the letter:
//   THE SCHEDULE.  tsync from fmod(time_sec - time_shift, slot_period) > slot_period / 4 with time_shift the FLOAT 0.8 (:510) and
//   slot_period a float (:514-515); TIME IS AN INPUT, the double clock_gettime would have given; a callback before sync is dropped whole
//   (:515-518); in_pos and frame_pos count samples and both restart at sync (:524); every sample of a callback is stored (:531-535: the
//   bound is commented out); the blocks due are those with in_pos >= frame_pos + block_size while frame_pos < num_samples (:541); the slot
//   ends when frame_pos >= num_samples (:545), the rest of that callback's samples are lost at the next sync; slot++ and decode_time at
//   each sync (:526-527); time_slot_start = (time_t) (time_sec - time_within_slot) (:520).
//   last_frame SURVIVES monitor_reset (monitor.c:134-138 clears num_blocks and max_mag alone): the first transforms of a slot see the
//   tail of the previous slot's samples; it is zeroed by decode_ft8_protocol (free + init: calloc, :75) and at create alone.  Hence
//   every analysis frame is a fixed window of (previous tail || this slot's samples): frame (block b, time_sub t) is the nfft samples
//   that end at b * block_size + (t + 1) * subblock_size, and every transform of a push is independent of the others.
//   monitor_process.  window[i] = fft_norm * hann_i(i, nfft) with sinf of the host libm ((float) M_PI * i / N in float, :11), made on
//   the host; timedata = window * last_frame (:170); per kept bin mag2 = i*i + r*r, db = 10.0f * log10f(1E-12f + mag2) (:180-181),
//   (int) (2 * db + 240) clamped to 0 .. 255 (:191-192); layout [block][time_sub][freq_sub][bin] (:147-194); max_mag the running
//   maximum of db from -120 (:196-197, :112, :137).
//   THE SYNC SCORE.  The integer neighbour differences of decode.c:96-119 (:159-182); `continue` below block 0, `break` out of the k
//   loop alone at num_blocks (:79-82); score /= num_average truncates (:123-124); the score is stored in an int16_t (:212, decode.h).
//   THE SELECTION.  Scan order time_sub, freq_sub, time_offset -10 .. 19, freq_offset (:203-210); score < min_score dropped (:214);
//   heap[0] evicted only by a strictly greater score (:219); heapify_up / _down and the final heap-sort swaps exactly as written: which of
//   several equal-minimum entries goes, and the order of equal scores in the output, are the heap's.  The record is the sequential loop's.
//   THE LIKELIHOODS.  WF_ELEM_MAG(x) = x * 0.5f - 120.0f (decode.h); max2 takes a >= b (:393-396); the bits of a symbol outside the
//   captured blocks are zero (:270-274, :296-301); sum and sum2 in index order in float, variance, sqrtf(24.0f / variance) (:312-327);
//   zero variance gives what the reference gives: inf, then 0 * inf = NaN.
// Defined here where the reference leaves it open:
//   * decode_time is (uint32) floor(time): tv_sec of the clock reading the caller hands in;
//   * stage 1's decode() takes no time: the DECODE event is the callback that ends the slot;
//   * the slot's samples are written without bound in the reference (malloc of slot_period * sample_rate floats): a callback longer than
//     MAX_NS samples is refused.
// REFUSED, nothing changed: snd_rate other than 12000 (20250 gives nfft 6480 / 1944: the transform's passes are general over 2^a 3^b 5^c
// but only the two sizes of 12000 are held to a golden, so the rate is refused, not faked), a protocol other than FT8 / FT4, a time that
// is not finite or outside 0 .. 2^40, a push before init.
#ifndef KG_FT8_H
#define KG_FT8_H
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "kg_nr.h"
#if defined(__HIPCC__)
#include "kg_libm.h"
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define KG_FT8_LOG10F(x) kg_libm::log10f_glibc(x)          // the host libm's log10f, bit for bit (kg_libm.h)
#else
#define KG_FT8_LOG10F(x) log10f(x)
#endif

namespace kg_ft8_cf {

enum { PROTO_FT8 = 0, PROTO_FT4 = 1 };                     // decode_ft8_init's `proto` (:567)
enum { TIME_OSR = 2, FREQ_OSR = 2, MAX_CAND = 140, MIN_SCORE = 10, LDPC_N = 174 };       // decode_ft8.c:73-80, constants.h:42
enum { F_MIN = 100, F_MAX = 3100 };                        // FT8.h:8-9
enum { FT8_ND = 58, FT8_LENGTH_SYNC = 7, FT8_NUM_SYNC = 3, FT8_SYNC_OFFSET = 36 };       // constants.h:22-26
enum { FT4_ND = 87, FT4_LENGTH_SYNC = 4, FT4_NUM_SYNC = 4, FT4_SYNC_OFFSET = 33 };       // constants.h:34-39
enum { TO_MIN = -10, TO_MAX = 20, NTO = TO_MAX - TO_MIN };                                // decode.c:208
enum { MAX_NS = 2048, MAX_NFFT = 3840, MAX_BINS = 481, MAX_BLOCKS = 156, MAX_SYNC_ROWS = 21 };
enum { REFUSED_RATE = -1, REFUSED_PROTO = -2, REFUSED_TIME = -3, REFUSED_NOT_INITED = -4 };
enum { EV_SLOT_START = 0, EV_DECODE = 1 };

#define KG_FT8_COSTAS {3, 1, 4, 0, 6, 5, 2}                                              /* constants.c:4 */
#define KG_FT4_COSTAS {{0, 1, 3, 2}, {1, 0, 2, 3}, {2, 3, 1, 0}, {3, 2, 0, 1}}            /* constants.c:5-10 */
#define KG_FT8_GRAY {0, 1, 3, 2, 5, 6, 4, 7}                                              /* constants.c:13 */
#define KG_FT4_GRAY {0, 1, 3, 2}                                                          /* constants.c:14 */

// ---- the sizes (decode_ft8_init, :569-578; monitor_init, monitor.c:57-63, :101-105)
struct cfg_t {
    int32_t protocol, sample_rate, block_size, subblock_size, nfft, min_bin, max_bin, num_bins, max_blocks, block_stride, num_samples, slot_blocks;
    float slot_period, symbol_period, fft_norm, pad;
};
inline cfg_t cfg_of(int protocol, int sample_rate)
{
    cfg_t c;
    memset(&c, 0, sizeof c);
    c.protocol = protocol; c.sample_rate = sample_rate;
    c.slot_period = protocol == PROTO_FT8 ? 15.0f : 7.5f;                                  // :569, constants.h:12, :15
    c.symbol_period = protocol == PROTO_FT4 ? 0.048f : 0.160f;                             // monitor.c:58
    c.num_samples = (c.slot_period - 0.4f) * sample_rate;                                  // :577
    c.block_size = (int) (sample_rate * c.symbol_period);                                  // monitor.c:60
    c.subblock_size = c.block_size / TIME_OSR;
    c.nfft = c.block_size * FREQ_OSR;
    c.fft_norm = 2.0f / c.nfft;
    c.max_blocks = (int) (c.slot_period / c.symbol_period);                                // monitor.c:101
    c.min_bin = (int) ((float) F_MIN * c.symbol_period);                                   // monitor.c:103-104: cfg->f_min is a float
    c.max_bin = (int) ((float) F_MAX * c.symbol_period) + 1;
    c.num_bins = c.max_bin - c.min_bin;
    c.block_stride = TIME_OSR * FREQ_OSR * c.num_bins;
    c.slot_blocks = (c.num_samples + c.block_size - 1) / c.block_size;                     // the passes of the loop of :541
    return c;
}
inline float hann_i(int i, int N) { float x = sinf((float) M_PI * i / N); return x * x; }   // monitor.c:9-13, host only
inline float window_at(const cfg_t &c, int i) { return c.fft_norm * hann_i(i, c.nfft); }   // monitor.c:70, host only: the device reads a table

// ---- monitor_process, one kept bin (monitor.c:179-197)
KG_NR_HD float sample_of(int16_t s) { return ((float) s) / 32768.0f; }                     // :533
KG_NR_HD float windowed(float w, float x) { return w * x; }                                // monitor.c:170
KG_NR_HD float db_of(float r, float i)
{
    float mag2 = (i * i) + (r * r);
    return 10.0f * KG_FT8_LOG10F(1E-12f + mag2);
}
KG_NR_HD unsigned char byte_of(float db)
{
    int scaled = (int) (2 * db + 240);
    return (unsigned char) ((scaled < 0) ? 0 : ((scaled > 255) ? 255 : scaled));
}
KG_NR_HD int src_bin_of(int min_bin, int bin, int freq_sub) { return ((min_bin + bin) * FREQ_OSR) + freq_sub; }   // monitor.c:179, bin from 0
// where the frame of time_sub t of the block at frame_pos starts among the slot's samples; below 0: the previous slot's tail
KG_NR_HD int frame_start(const cfg_t &c, int frame_pos, int t) { return frame_pos + (t + 1) * c.subblock_size - c.nfft; }

// ---- the sync score (decode.c:63-190).  rd(m, k, f): the byte of the candidate's block (m, k) at bin freq_offset + f
struct cand_t { int16_t score, time_offset, freq_offset; uint8_t time_sub, freq_sub; };    // ftx_candidate_t (decode.h)
template <typename RD> KG_NR_HD int sync_score(int protocol, int time_offset, int num_blocks, const unsigned char *costas, RD rd)
{
    const int ft4 = protocol == PROTO_FT4;
    const int NUM = ft4 ? (int) FT4_NUM_SYNC : (int) FT8_NUM_SYNC, LEN = ft4 ? (int) FT4_LENGTH_SYNC : (int) FT8_LENGTH_SYNC, OFF = ft4 ? (int) FT4_SYNC_OFFSET : (int) FT8_SYNC_OFFSET;
    const int top = ft4 ? 3 : 7;
    int score = 0;
    int num_average = 0;
    for (int m = 0; m < NUM; ++m) {
        for (int k = 0; k < LEN; ++k) {
            int block = (ft4 ? 1 : 0) + (OFF * m) + k;                                     // :76, :142
            int block_abs = time_offset + block;
            if (block_abs < 0) continue;
            if (block_abs >= num_blocks) break;
            int sm = ft4 ? costas[m * FT4_LENGTH_SYNC + k] : costas[k];                    // :95, :153
            if (sm > 0) { score += (int) rd(m, k, sm) - (int) rd(m, k, sm - 1); ++num_average; }
            if (sm < top) { score += (int) rd(m, k, sm) - (int) rd(m, k, sm + 1); ++num_average; }
            if ((k > 0) && (block_abs > 0)) { score += (int) rd(m, k, sm) - (int) rd(m, k - 1, sm); ++num_average; }
            if (((k + 1) < LEN) && ((block_abs + 1) < num_blocks)) { score += (int) rd(m, k, sm) - (int) rd(m, k + 1, sm); ++num_average; }
        }
    }
    if (num_average > 0) score /= num_average;
    return score;
}
KG_NR_HD int sync_block(int protocol, int m, int k) { return protocol == PROTO_FT4 ? 1 + FT4_SYNC_OFFSET * m + k : FT8_SYNC_OFFSET * m + k; }
KG_NR_HD int num_tones(int protocol) { return protocol == PROTO_FT4 ? 4 : 8; }
KG_NR_HD int num_freq_offsets(const cfg_t &c) { return c.num_bins - num_tones(c.protocol) + 1; }       // :210
KG_NR_HD int num_hyp(const cfg_t &c) { return TIME_OSR * FREQ_OSR * NTO * num_freq_offsets(c); }
// hypothesis h in scan order (:203-210)
KG_NR_HD cand_t hyp_of(const cfg_t &c, int h, int score)
{
    const int nfo = num_freq_offsets(c);
    cand_t x;
    x.freq_offset = (int16_t) (h % nfo); h /= nfo;
    x.time_offset = (int16_t) (TO_MIN + h % NTO); h /= NTO;
    x.freq_sub = (uint8_t) (h % FREQ_OSR); h /= FREQ_OSR;
    x.time_sub = (uint8_t) h;
    x.score = (int16_t) score;
    return x;
}
// get_cand_mag (:54-61) plus a block and a bin: the index into mag[]
KG_NR_HD int mag_index(const cfg_t &c, int block_abs, int time_sub, int freq_sub, int bin)
{
    return ((block_abs * TIME_OSR + time_sub) * FREQ_OSR + freq_sub) * c.num_bins + bin;
}

// ---- the heap (decode.c:403-454), exactly as written
KG_NR_HD void heapify_down(cand_t *heap, int heap_size)
{
    int current = 0;
    while (true) {
        int left = 2 * current + 1;
        int right = left + 1;
        int smallest = current;
        if ((left < heap_size) && (heap[left].score < heap[smallest].score)) smallest = left;
        if ((right < heap_size) && (heap[right].score < heap[smallest].score)) smallest = right;
        if (smallest == current) break;
        cand_t tmp = heap[smallest];
        heap[smallest] = heap[current];
        heap[current] = tmp;
        current = smallest;
    }
}
KG_NR_HD void heapify_up(cand_t *heap, int heap_size)
{
    int current = heap_size - 1;
    while (current > 0) {
        int parent = (current - 1) / 2;
        if (!(heap[current].score < heap[parent].score)) break;
        cand_t tmp = heap[parent];
        heap[parent] = heap[current];
        heap[current] = tmp;
        current = parent;
    }
}
// one passing hypothesis of the scan (:217-232)
KG_NR_HD void heap_take(cand_t *heap, int &heap_size, int num_candidates, const cand_t &candidate)
{
#ifdef KG_FT8_MUT_EVICT                                      /* tests/test_ft8_cpu.py: the golden must notice an eviction on an equal score */
    if ((heap_size == num_candidates) && (candidate.score >= heap[0].score)) {
#else
    if ((heap_size == num_candidates) && (candidate.score > heap[0].score)) {
#endif
        --heap_size;
        heap[0] = heap[heap_size];
        heapify_down(heap, heap_size);
    }
    if (heap_size < num_candidates) {
        heap[heap_size] = candidate;
        ++heap_size;
        heapify_up(heap, heap_size);
    }
}
KG_NR_HD void heap_sort(cand_t *heap, int heap_size)                                        // :239-251
{
    int len_unsorted = heap_size;
    while (len_unsorted > 1) {
        cand_t tmp = heap[len_unsorted - 1];
        heap[len_unsorted - 1] = heap[0];
        heap[0] = tmp;
        len_unsorted--;
        heapify_down(heap, len_unsorted);
    }
}
// The scan of ftx_find_candidates on the hypotheses that passed min_score, in scan order: entry e is (hypothesis index) | (score << 16);
// a hypothesis index is below 2^16 (56880 at most).  One lane's work on the device, as WSPR's peak_list() is.
KG_NR_HD uint32_t pass_entry(int h, int score) { return (uint32_t) h | ((uint32_t) (uint16_t) (int16_t) score << 16); }
KG_NR_HD int heap_of_list(const cfg_t &c, const uint32_t *list, int n, int num_candidates, cand_t *heap)
{
    int heap_size = 0;
    for (int e = 0; e < n; e++) {
        const uint32_t v = list[e];
        heap_take(heap, heap_size, num_candidates, hyp_of(c, (int) (v & 0xffffu), (int16_t) (uint16_t) (v >> 16)));
    }
    heap_sort(heap, heap_size);
    return heap_size;
}

// ---- the likelihoods (decode.c:256-328, :457-485)
KG_NR_HD float elem_mag(unsigned char x) { return (float) (x) * 0.5f - 120.0f; }            // WF_ELEM_MAG
KG_NR_HD float max2(float a, float b) { return (a >= b) ? a : b; }
KG_NR_HD float max4(float a, float b, float c, float d) { return max2(max2(a, b), max2(c, d)); }
KG_NR_HD int num_data_syms(int protocol) { return protocol == PROTO_FT4 ? (int) FT4_ND : (int) FT8_ND; }
KG_NR_HD int sym_idx_of(int protocol, int k)                                                // :265, :291
{
    return protocol == PROTO_FT4 ? k + ((k < 29) ? 5 : ((k < 58) ? 9 : 13)) : k + ((k < 29) ? 7 : 14);
}
// data symbol k of a candidate: its 3 (FT8) or 2 (FT4) unnormalised bits into logl; wf(f): the byte of the symbol's block at freq_offset + f
template <typename WF> KG_NR_HD void extract_symbol(int protocol, const unsigned char *gray, WF wf, float *logl)
{
    if (protocol == PROTO_FT4) {
        float s2[4];
        for (int j = 0; j < 4; ++j) s2[j] = elem_mag(wf(gray[j]));
        logl[0] = max2(s2[2], s2[3]) - max2(s2[0], s2[1]);
        logl[1] = max2(s2[1], s2[3]) - max2(s2[0], s2[2]);
    } else {
        float s2[8];
        for (int j = 0; j < 8; ++j) s2[j] = elem_mag(wf(gray[j]));
        logl[0] = max4(s2[4], s2[5], s2[6], s2[7]) - max4(s2[0], s2[1], s2[2], s2[3]);
        logl[1] = max4(s2[2], s2[3], s2[6], s2[7]) - max4(s2[0], s2[1], s2[4], s2[5]);
        logl[2] = max4(s2[1], s2[3], s2[5], s2[7]) - max4(s2[0], s2[2], s2[4], s2[6]);
    }
}
KG_NR_HD float norm_factor_of(const float *log174)                                          // :312-323: index order, one lane, no tree
{
    float sum = 0;
    float sum2 = 0;
    for (int i = 0; i < LDPC_N; ++i) {
        sum += log174[i];
        sum2 += log174[i] * log174[i];
    }
    float inv_n = 1.0f / LDPC_N;
    float variance = (sum2 - (sum * sum * inv_n)) * inv_n;
    return sqrtf(24.0f / variance);
}
KG_NR_HD float freq_hz_of(const cfg_t &c, const cand_t &x) { return (c.min_bin + x.freq_offset + (float) x.freq_sub / FREQ_OSR) / c.symbol_period; }   // decode_ft8.c:229
KG_NR_HD float time_sec_of(const cfg_t &c, const cand_t &x) { return (x.time_offset + (float) x.time_sub / TIME_OSR) * c.symbol_period; }              // :230
KG_NR_HD float snr_of(const cand_t &x, float snr_adj) { return x.score * 0.5f + snr_adj; }                                                            // :303

// ---- the slot end on the host (the twin the kernels are held to): ftx_find_candidates and, per candidate, ftx_decode_candidate up to log174
struct slot_t {
    int32_t ncand;
    cand_t cand[MAX_CAND];
    float freq_hz[MAX_CAND], time_sec[MAX_CAND], snr[MAX_CAND];
    float log174[MAX_CAND][LDPC_N];
};
inline int score_of(const cfg_t &c, const unsigned char *mag, int num_blocks, const cand_t &x)
{
    static const unsigned char c8[7] = KG_FT8_COSTAS, c4[4][4] = KG_FT4_COSTAS;
    return sync_score(c.protocol, x.time_offset, num_blocks, c.protocol == PROTO_FT4 ? &c4[0][0] : c8, [&](int m, int k, int f) {
        return mag[mag_index(c, x.time_offset + sync_block(c.protocol, m, k), x.time_sub, x.freq_sub, x.freq_offset + f)];
    });
}
inline void likelihood_of(const cfg_t &c, const unsigned char *mag, int num_blocks, const cand_t &x, float *log174)
{
    static const unsigned char g8[8] = KG_FT8_GRAY, g4[4] = KG_FT4_GRAY;
    const int per = c.protocol == PROTO_FT4 ? 2 : 3;
    for (int k = 0; k < num_data_syms(c.protocol); ++k) {
        const int block = x.time_offset + sym_idx_of(c.protocol, k);
        float *logl = log174 + per * k;
        if ((block < 0) || (block >= num_blocks)) { for (int j = 0; j < per; j++) logl[j] = 0; continue; }
        extract_symbol(c.protocol, c.protocol == PROTO_FT4 ? g4 : g8, [&](int f) { return mag[mag_index(c, block, x.time_sub, x.freq_sub, x.freq_offset + f)]; }, logl);
    }
    const float norm_factor = norm_factor_of(log174);
    for (int i = 0; i < LDPC_N; ++i) log174[i] *= norm_factor;
}
inline void slot_end(const cfg_t &c, const unsigned char *mag, int num_blocks, int num_candidates, int min_score, float snr_adj, slot_t &out)
{
    memset(&out, 0, sizeof out);
    std::vector<uint32_t> list;
    const int nh = num_hyp(c);
    for (int h = 0; h < nh; h++) {
        const int score = (int16_t) score_of(c, mag, num_blocks, hyp_of(c, h, 0));
        if (score < min_score) continue;
        list.push_back(pass_entry(h, score));
    }
    out.ncand = heap_of_list(c, list.data(), (int) list.size(), num_candidates, out.cand);
    for (int i = 0; i < out.ncand; i++) {
        out.freq_hz[i] = freq_hz_of(c, out.cand[i]); out.time_sec[i] = time_sec_of(c, out.cand[i]); out.snr[i] = snr_of(out.cand[i], snr_adj);
        likelihood_of(c, mag, num_blocks, out.cand[i], out.log174[i]);
    }
}

// ---- the schedule
struct state_t {
    int32_t inited, protocol, tsync, in_pos, frame_pos, num_blocks, parity, pad;
    uint32_t slot, decode_time;
    int64_t slot_start;
    cfg_t cfg;
};
// what one callback asks of the device, in order: COPY n samples of the callback (from its first) to in_pos a of the slot of `parity`;
// BLOCK a of that slot is due (src: its frame_pos); END: the slot of `parity`, number n, ends with a blocks
enum { OP_COPY = 0, OP_BLOCK = 1, OP_END = 2 };
struct op_t { int32_t kind, parity, a, n; int64_t src; };
struct ev_t { int32_t cb, kind, a, b; int64_t t; };        // SLOT_START: a the slot number, b decode_time, t time_slot_start; DECODE: a num_blocks, b the slot number
struct sched_t {
    std::vector<op_t> ops;
    std::vector<ev_t> evs;
    int32_t nend = 0;
};
inline bool time_ok(double t) { return t >= 0.0 && t <= 1099511627776.0; }                   // finite too: a NaN fails both
// one callback of decode_ft8_samples (:503-559) with ns samples whose first is sample `base` of the push, at clock reading time_sec
inline void sched_callback(state_t &w, sched_t &p, int cb, int64_t base, int ns, double time_sec)
{
    const cfg_t &c = w.cfg;
    if (!w.tsync) {
        const float time_shift = 0.8;
        double time_within_slot = fmod(time_sec - time_shift, c.slot_period);
        if (time_within_slot > c.slot_period / 4) return;
        w.slot_start = (int64_t) (time_sec - time_within_slot);
        w.in_pos = w.frame_pos = 0;
        w.decode_time = (uint32_t) (int64_t) floor(time_sec);
        w.slot++;
        w.tsync = 1;
        p.evs.push_back(ev_t{cb, EV_SLOT_START, (int32_t) w.slot, (int32_t) w.decode_time, w.slot_start});
    }
    p.ops.push_back(op_t{OP_COPY, w.parity, w.in_pos, ns, base});
    w.in_pos += ns;
    const int block_size = c.block_size;
    if (w.in_pos < w.frame_pos + block_size) return;
    while (w.in_pos >= w.frame_pos + block_size && w.frame_pos < c.num_samples) {
        if (w.num_blocks < c.max_blocks) {                                                  // monitor.c:144
            p.ops.push_back(op_t{OP_BLOCK, w.parity, w.num_blocks, 0, (int64_t) w.frame_pos});
            w.num_blocks++;
        }
        w.frame_pos += block_size;
    }
    if (w.frame_pos < c.num_samples) return;
    p.evs.push_back(ev_t{cb, EV_DECODE, w.num_blocks, (int32_t) w.slot, w.slot_start});
    p.ops.push_back(op_t{OP_END, w.parity, w.num_blocks, (int32_t) w.slot, 0});
    p.nend++;
    w.num_blocks = 0;                                                                       // monitor_reset; max_mag is the device's
    w.tsync = 0;
    w.parity ^= 1;                                                                          // ours: the next slot's samples and bytes go to the other half
}
// decode_ft8_init (:561-596), also decode_ft8_protocol (:609-617): everything of the connection begins again, last_frame zeroed
inline int cmd_init(state_t &w, int protocol, double snd_rate)
{
    if (!(snd_rate == 12000.0)) return REFUSED_RATE;
    if (protocol != PROTO_FT8 && protocol != PROTO_FT4) return REFUSED_PROTO;
    memset(&w, 0, sizeof w);
    w.inited = 1;
    w.protocol = protocol;
    w.cfg = cfg_of(protocol, (int) snd_rate);
    if (w.cfg.slot_blocks > w.cfg.max_blocks || w.cfg.nfft > MAX_NFFT || w.cfg.num_bins > MAX_BINS) { memset(&w, 0, sizeof w); return REFUSED_RATE; }
    return 0;
}

}  // namespace kg_ft8_cf
#endif
