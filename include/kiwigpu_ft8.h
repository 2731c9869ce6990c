/* kiwigpu_ft8.h -- the FT8 / FT4 extension (extensions/FT8/, ft8_lib), stage 1: from the real-samples tap (decode_ft8_samples,
 * ft8_lib/decode_ft8.c:503-559) to log174, the normalised soft bits of every candidate.  Included by kiwigpu.h; a host includes
 * kiwigpu.h alone.
 *
 * Per connection a decode_ft8_t with its monitor_t (common/monitor.c:55-203, WF_ELEM_T uint8_t): the sync to the 15 s (FT8) or 7.5 s
 * (FT4) slot, two windowed transforms of 3840 (1152) samples per symbol into the waterfall bytes [block][time_sub][freq_sub][bin], and
 * at the end of a slot ftx_find_candidates (ft8/decode.c:192-254: about 57 000 Costas sync scores, the min-heap of the 140 best) and per
 * candidate ft8 / ft4_extract_likelihood with ftx_normalize_logl (:256-328).  Stage 2 -- bp_decode, the CRC and the message -- is not
 * here: it starts from kg_ft8_slot.  csrc/kg_ft8.h is the one definition for device and host, in the reference's operand types, and
 * cites the reference item by item; it lists what is kept to the letter.
 *
 * TIME IS AN INPUT: every callback of a push carries the double that clock_gettime would have given (seconds, :512-513); no sample
 * drives the schedule.  A callback before the sync is dropped whole; the callback that ends a slot loses its remaining samples.
 * last_frame survives the end of a slot: a slot's first transforms see the previous slot's tail; kg_ft8_init zeroes it.
 * SNR_adj (ft8_conf.SNR_adj, :303) is an input too: kg_ft8_set_snr_adj, -22 until set (FT8.cpp:312).
 * Every entry point here synchronises unless it says otherwise.
 * REFUSED, nothing changed (KG_ERR_INVALID unless stated): a null handle; a connection out of range or listed twice; snd_rate other than
 * 12000; a protocol other than 0 / 1; ns outside 1 .. KG_FT8_MAX_NS; a time that is not finite or outside 0 .. 2^40; a push before
 * kg_ft8_init (KG_ERR_STATE); a push in which one connection would end two slots; more events or slots than the caller's arrays hold. */
#ifndef KIWIGPU_FT8_H
#define KIWIGPU_FT8_H

typedef struct kg_ft8 kg_ft8;
#define KG_FT8_MAX_CAND 140                                /* kMax_candidates, decode_ft8.c:74 */
#define KG_FT8_MIN_SCORE 10                                /* kMin_score, :73 */
#define KG_FT8_LDPC_N 174                                  /* FTX_LDPC_N, ft8/constants.h:42 */
#define KG_FT8_MAX_NS 2048                                 /* samples of one callback at most */
#define KG_FT8_MAX_NFFT 3840
#define KG_FT8_MAX_WF 178932                               /* waterfall bytes of a connection at most: 93 blocks x 4 x 481 bins */
enum { KG_FT8_PROTO_FT8 = 0, KG_FT8_PROTO_FT4 = 1 };       /* decode_ft8_init's proto */
enum { KG_FT8_EV_SLOT_START = 0, KG_FT8_EV_DECODE = 1 };

typedef struct kg_ft8_ev {                 /* SLOT_START (:520-528): a the slot number, b decode_time, t time_slot_start; DECODE (:549-554): a num_blocks, b the slot number, t time_slot_start */
    int32_t conn, cb, kind, a, b, pad; int64_t t;          /* cb: the callback of the push */
} kg_ft8_ev;
typedef struct kg_ft8_cand {               /* ftx_candidate_t (ft8/decode.h) and decode_ft8.c:229-230, :303 */
    int16_t score, time_offset, freq_offset; uint8_t time_sub, freq_sub;
    float freq_hz, time_sec, snr;
} kg_ft8_cand;
typedef struct kg_ft8_slot {               /* one ended slot: the candidates in the order ftx_find_candidates leaves them; zeros behind ncand */
    int32_t conn, due, ncand, num_blocks, protocol, slot; float max_mag; int32_t pad;
    kg_ft8_cand cand[KG_FT8_MAX_CAND];
    float log174[KG_FT8_MAX_CAND][KG_FT8_LDPC_N];
} kg_ft8_slot;
typedef struct kg_ft8_info {               /* decode_ft8_t / monitor_t, what this stage keeps of them */
    int32_t inited, protocol, tsync, in_pos, frame_pos, num_blocks, parity, last_blocks;
    int32_t block_size, nfft, num_bins, min_bin, max_blocks, num_samples, slot_blocks, block_stride;
    uint32_t slot, decode_time; int64_t slot_start;
    float max_mag, last_max_mag;           /* of the slot under way, and of the slot that ended last */
} kg_ft8_info;

/* nconn decode_ft8_t, not initialised, last_frame zeroed (calloc, monitor.c:75); 1 .. 64 */
int kg_ft8_create(kg_ctx *ctx, int nconn, kg_ft8 **out);
/* decode_ft8_free (:598-607) of every connection; drains the context's stream first */
void kg_ft8_destroy(kg_ft8 *q);
/* ft8_conf.SNR_adj (:303) of every connection; finite */
int kg_ft8_set_snr_adj(kg_ft8 *q, float snr_adj);
/* decode_ft8_init (:561-596) and decode_ft8_protocol (:609-617: free + init): the connection begins again, not synced, slot 0, no
 * block, last_frame zeroed.  Enqueues the clearing; does not synchronise. */
int kg_ft8_init(kg_ft8 *q, int conn, int protocol, double snd_rate);
/* decode_ft8_samples (:503-559) for ncb[i] callbacks of ns samples per listed connection: entry i's samples at samples + i * sample_stride, its
 * callbacks' clock readings at times + i * time_stride (a list of one has no strides).  The events in list order, then callback order.
 * Per slot that ends, in list order, one kg_ft8_slot (num_candidates 140, min_score 10): the monitor launch of the push, then sync
 * scores, selection and likelihoods behind it on the same stream with no host read between them. */
int kg_ft8_push(kg_ft8 *q, const int32_t *conns, int nconn, const int32_t *ncb, int ns, const int16_t *samples, size_t sample_stride, const double *times,
                size_t time_stride, kg_ft8_ev *evs, int max_events, int32_t *nevents, kg_ft8_slot *slots, int max_slots, int32_t *nslots);
/* the schedule of that push (:509-546) on copies of the connections' states: nothing changes.  Counts may be null. */
int kg_ft8_plan(kg_ft8 *q, const int32_t *conns, int nconn, const int32_t *ncb, int ns, const double *times, size_t time_stride, int32_t *nblocks,
                int32_t *nevents, int32_t *nslots);
/* info; last_frame [nfft]: the analysis frame as monitor_process left it (monitor.c:157-165); mag: the waterfall bytes of the slot under way (previous 0:
 * num_blocks * block_stride of them) or of the slot that ended last (previous 1: last_blocks * block_stride).  Each may be null. */
int kg_ft8_state(kg_ft8 *q, int conn, kg_ft8_info *info, float *last_frame, uint8_t *mag, int previous);
/* The load path: the slot-end chain on a waterfall handed in -- ftx_find_candidates(wf, num_candidates, heap, min_score) (decode.c:192-254) and the
 * likelihoods of its candidates -- with mag [num_blocks][2][2][num_bins] of `protocol` at 12000 Hz.  num_blocks 1 .. max_blocks,
 * num_candidates 1 .. 140, min_score -32768 .. 32767.  Nothing of the connection is touched: the bytes go to a third waterfall of their own; max_mag of the record is -120. */
int kg_ft8_load_wf(kg_ft8 *q, int conn, int protocol, int num_blocks, const uint8_t *mag, int num_candidates, int min_score, kg_ft8_slot *slot);

/* ---- The receiver bank (kg_rxbank): FT8 is the third holder of the real-samples task tap (ext_register_receive_real_samps_task, FT8.cpp:203),
 * fed as FAX and the CW decoder are: while a receiver is started and its blocks go on the mono list, every sound block of a step is one
 * callback of 512 int16 samples read in place, with the clock reading of the last kg_rxbank_ft8_set_now.  The launches go on the bank's
 * tail stream ahead of the step's end; the slot-end chain follows the monitor launch with no host wait.  A bank never told holds nothing
 * for it and enqueues what it always did.  Join and leave give the receiver a fresh, uninitialised connection. */
struct kg_rxbank;
/* decode_ft8_init / decode_ft8_protocol (:561-617) of receiver rx */
int kg_rxbank_ft8_init(struct kg_rxbank *bank, int rx, int protocol, double snd_rate);
/* ext_register_receive_real_samps_task (FT8.cpp:203): refused (KG_ERR_STATE) before kg_rxbank_ft8_init, and while FAX or the CW decoder is
 * started on the receiver -- the tap holds one task; they are refused beside a started FT8 */
int kg_rxbank_ft8_start(struct kg_rxbank *bank, int rx);
/* ext_unregister_receive_real_samps_task (FT8.cpp:153): the connection keeps its state */
int kg_rxbank_ft8_stop(struct kg_rxbank *bank, int rx);
/* what clock_gettime answers (:512-513) during every later step; finite, 0 .. 2^40 */
int kg_rxbank_ft8_set_now(struct kg_rxbank *bank, double now);
/* the bank's object (NULL until the extension was named): for kg_ft8_state and kg_ft8_set_snr_adj (:303) alone -- the bank feeds it */
kg_ft8 *kg_rxbank_ft8(struct kg_rxbank *bank);
/* The last step's output (:549-554), valid once the step has been waited for: the events in receiver order (conn the receiver, cb the
 * sound block of the step), and the slot records on the device, record k the receiver rx_of_slot[k]'s.  Returns the number of records. */
int kg_rxbank_ft8_out(struct kg_rxbank *bank, kg_ft8_slot **d_slots, kg_ft8_ev *evs, int max_events, int32_t *nevents, int32_t *rx_of_slot, int max_slots);

#endif
