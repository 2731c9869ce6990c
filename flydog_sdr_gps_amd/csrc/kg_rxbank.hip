// kg_rxbank.hip -- a bank of virtual receivers stepped with ONE call (BASELINE configs[3]).
//
// In the reference every connection has a waterfall coroutine and a sound coroutine that loop over what the data pump and
// the FPGA hand them (rx/data_pump.cpp:292-341 data_pump(); rx/rx_sound.cpp:333-601 the c2s_sound() loop: in_samps ->
// CFastFIR -> S-meter / AGC / demod -> compression -> snd_pkt; rx/rx_waterfall.cpp:930-1170 c2s_waterfall() -> sample_wf()
// -> compute_frame() -> wf_pkt_t).  A bank is nrx such connections on one GPU, fed from one block of ADC samples per step:
//
//   waterfall of receiver k   IQ_MIXER + wf1 CIC (kg_ddc) in the sampler mode the reference chose for it
//                               one-shot    CmdWFReset + 8192 outputs, the non-overlapped frame (rx_waterfall.cpp:1005-1041)
//                               overlapped  continuous sampler, the frame = the ring's newest 8192 outputs read at the
//                                           synchronised write address (:967-983, CmdGetWFContSamps) -- the mode sample_wf()
//                                           switches to when a frame takes longer to fill than two display periods
//                             -> window + FFT + power + pixels + dB + u8 row (kg_wf) -> wf_pkt_t, ADPCM (kg_wf_packets_dev)
//   audio of receiver k       IQ_MIXER + rx1 / rx2 CIC + CICF (kg_rxddc) -> rx_iq_t records -> snd_service() unpack
//                             -> CFastFIR (kg_fir) -> S-meter + CAgc + detector (kg_post) -> IMA ADPCM (kg_adpcm)
//
// The per-seam objects are the bank's and are configured with their own entry points (kg_rxbank_ddc() ... kg_rxbank_adpcm());
// what the bank adds is the step: which kernel goes on which of its three streams (waterfall chain, audio chain, the two
// sequential coders), the events between them, and ONE upload per step for the small tables of all stages.  A step is
//   plan      bank_plan_step decides what the step is -- lists, rows, ring moves, frames, every next value -- from host state alone
//   enqueue   bank_pass calls the entry points as the plan says, twice: first in the context's PLAN mode (kg_common.h, kg_arena:
//             tables collected, nothing launched, no state advanced), then -- behind the one transfer -- for real
//   commit    bank_commit moves the plan's next values and maps into the bank, after a real pass that succeeded
#include "kg_common.h"
#include "kg_nb.h"
#include "kg_spec.h"

#include <chrono>
#include <math.h>
#include <stdlib.h>
#include <mutex>
#include <vector>

// Loran-C in a bank: a GRI is BANK_LO_MIN_SPG samples or more, so a channel has at most 4 B + 4 runs (and rows) in a step of B sound
// blocks: 4 B whole GRIs, a partial one, and the cuts where samp and the unsigned difference wrap
#define BANK_LO_MIN_SPG 128.0
#define BANK_LO_RUNS(blocks_) (4 * (size_t) (blocks_) + 4)
// FAX in a bank: a line is BANK_FAX_MIN_SPL samples or more and an image BANK_FAX_MAX_WIDTH pixels or fewer, which bounds the lines
// and the row bytes of a step (kg_fax_max_lines' rule: a block gives at most 1026 picks)
#define BANK_FAX_MIN_SPL 1024
#define BANK_FAX_MAX_WIDTH 4096
#define BANK_SLOTS KG_RXBANK_SLOTS         // step-table slots in flight (a slot is reused BANK_SLOTS steps later)
#define BANK_RING_PAIRS (8 * KG_WF_NFFT)   // an overlapped receiver's sample ring (iq_t pairs); >= 2 frames
#define BANK_PKT_STRIDE 1056               // >= KG_WF_PKT_MAX, a multiple of 16

struct bank_move { int row, src, dst, cnt; };         // iq_t pairs inside one receiver's ring

// The ring of an overlapped receiver is linear: when the next step's outputs would run past its end, the newest
// 8192 - m pairs (m = outputs per step) move to the front and writing goes on behind them, so that a frame is always
// 8192 consecutive pairs.  One workgroup per move; source and destination never overlap (ring >= 2 frames).
__global__ __launch_bounds__(256) void rxbank_move_kernel(short2 *__restrict__ iq, long stride, const bank_move *__restrict__ tab)
{
    const bank_move m = tab[blockIdx.x];
    short2 *row = iq + (long) m.row * stride;
    for (int i = threadIdx.x; i < m.cnt; i += 256) row[m.dst + i] = row[m.src + i];
}

// the noise-blanker command state of snd_t and wf_inst_t (rx/rx_sound_cmd.cpp:454-501, :660-672)
struct bank_nb_cmd {
    int algo, snd_en[4], wf_en[4];
    float snd_param[4][8], wf_param[4][8];
    int wf_change[4], wf_setup;
};

// One receiver.  Connections come and go one at a time (rx/rx_sound.cpp:264-269: every c2s_sound() has its own CFastFIR position,
// sequence number and loop): a receiver is stepped while `active`; its audio DDC / CFastFIR were reset when IT joined, so what a
// step yields -- records, sound blocks -- is per receiver.
struct bank_rx {
    // the connection's: kg_rxbank_join starts all of these over
    char active = 1;
    uint32_t snd_seq = 0;                       // sound blocks emitted since it joined (the seq of its packets)
    int32_t last_nrec = 0, last_nfir = 0;       // the last step's counts (kg_rxbank_audio_map)
    char wf_set = 0;
    long ring_w = 0, ring_total = 0;            // overlapped: next write position, outputs written since the sampler was set
    // the audio spectrum (`SET spc_=2`, rx/rx_sound.cpp:175-220): s->specAF_FFT != NULL, the host's mirror of s->specAF_instance /
    // s->isChanNull and the kg_post mode commands it has seen (each clears the mirror)
    char spec_on = 0;
    kg_spec::emit_t spec_mirror = {KG_SPEC_PASSBAND};
    uint32_t spec_cmds = 0;
    bank_nb_cmd nbc = {};
    // the settings a join leaves alone
    int decim = 0; char overlapped = 0;         // kg_rxbank_set_wf
    char little_endian = 0;                     // s->little_endian
    kg_wf_pkt_info pkt = {0, 0, 0, 1};
};

// a sound block's channel lists, in the order they are enqueued
enum { BL_POST = 0, BL_NULL, BL_REAL, BL_IQ_BE, BL_IQ_LE, BL_N };

// What one step is.  bank_plan_step fills it from host state; both enqueue passes read it; bank_commit moves it into the bank.
// The vectors keep their capacity: a step allocates nothing.
struct bank_plan {
    // the active list: entry i is receiver act[i]
    std::vector<int32_t> act, nrec, nfir, mode;         // rx_iq_t records and CFastFIR outputs of the step, the kg_post mode
    std::vector<uint8_t> enabled;                       // per RECEIVER: active
    std::vector<char> sam_null;                         // runs kg_post in channel-null SAM this step (SAM_mparam & 3)
    int nrec_max, nfir_max;
    std::vector<int32_t> nb_list, nb_cnt;               // the blanked receivers (NB_STD) and their record counts
    // the audio spectrum's rows in emission order, receiver by receiver; CFastFIR's request per entry
    int nspec; bool any_pb;
    std::vector<int32_t> spec_rx, spec_inst, spec_blk, pb_inst, pb_n, pb_base;
    std::vector<int32_t> null_row;                      // [entry][blocks_max]: the channel-null row of a sound block, or -1
    std::vector<int32_t> null_each, null_inst;          // constants: 512 samples, KG_SPEC_CHAN_NULL
    // per sound block: list j of block blk is blk_chan[blk_at[BL_N * blk + j] .. blk_at[BL_N * blk + j + 1]); beside a BL_NULL
    // entry its row count and row
    std::vector<int32_t> blk_chan, blk_at, blk_null_n, blk_null_base;
    int at(int blk, int j) const { return blk_at[(size_t) BL_N * blk + j]; }
    int count(int blk, int j) const { return blk_at[(size_t) BL_N * blk + j + 1] - blk_at[(size_t) BL_N * blk + j]; }
    // the waterfall chain: ring moves, where each entry's DDC writes, the frame table
    std::vector<bank_move> moves;
    std::vector<int64_t> out_off, max_out;
    int nframes, wf_unset;                              // wf_unset: the first active receiver without a waterfall setting, or -1
    std::vector<int32_t> chan_of; std::vector<uint64_t> frame_off; std::vector<kg_wf_pkt_info> pkt_step;
    // the next values of what the step advances, per entry
    std::vector<long> ring_w, ring_total;
    std::vector<kg_spec::emit_t> mirror; std::vector<uint32_t> cmds;
    // what the entry points hand back
    std::vector<int32_t> got_nrec, got_nfir, pkt_bytes;
    std::vector<int64_t> h_nw;
};

// ---- the extensions: one record each, holding ALL the bank keeps for it.  A record's object and device buffers are made by the first
// kg_rxbank_<ext>_* call (bank_<ext>_ensure): a bank that was never told holds nothing for the extension and enqueues what it always
// did.  `on` is per receiver; `plan` is the step being made (the plan pass writes nothing else, the enqueue fills in what the entry
// point hands back); `last` is the last step's maps, moved there by the commit.

// The FFT extension (extensions/FFT/FFT.cpp; kg_fftext).  While a receiver's function is on, both filters store their filtered spectra
// (receive_FFT(POST_FILTERED), fastfir.cpp:293-302) and the extension runs ONCE per step over the step's blocks, on the tail stream.
struct bank_fx {
    kg_fftext *obj; double rate;                        // rate: kg_rxbank_fftext_set_rate's, kept for an object made later
    // d_post, in blocks of 1024 complex floats (the taps of a CFastFIR call lie by LIST ENTRY): [nrx][blocks_max] m_PassbandFIR's
    // blocks of the step, entry i of the step's active list; then [blocks_max][nrx] m_chan_null_FIR's, entry p of sound block blk's list
    kg_dbuf<float2> d_post; size_t stride;
    kg_dbuf<unsigned char> d_rows; size_t max;          // [max][1024] u8: the step's rows in map order
    std::vector<char> on;                               // run != FUNC_OFF
    struct {
        // the entries: receiver, blocks, instance, where the spectra lie in d_post, the entry's first sound block
        std::vector<int32_t> list, nblk, inst, row, blk0;
        std::vector<int32_t> nullpos;                   // per sound block: entries of its channel-null list so far
        std::vector<int32_t> rx, ent, blk, bin; int n;  // handed back: the rows
    } plan;
    struct { std::vector<int32_t> rx, blk, bin; int n; } last;        // kg_rxbank_fftext_map
};

// The IQ display (extensions/IQ_display/iq_display.cpp; kg_iqd).  While a receiver has run on and is not in NBFM, its CFastFIR output
// of the step (receive_iq_pre_agc, rx_sound.cpp:668-669) feeds it: ONE launch per step over all such receivers and their sound
// blocks, on the tail stream.
struct bank_iq {
    kg_iqd *obj;
    kg_dbuf<unsigned char> d_rows; size_t cap; int max_rows;          // the step's rows back to back: (512 B + 16384) * 4 bytes a receiver
    kg_dbuf<kg_iqd_status> d_st;                                      // a record per (entry, sound block) of the step's call
    std::vector<char> on;                               // `SET run=` (ext_register_receive_iq_samps)
    struct {
        std::vector<int32_t> list, nblk, inst, row;     // the entries: receiver, blocks, instance (0), the receiver's row of d_firo
        std::vector<kg_iqd_row> rows; std::vector<int32_t> sent; int n;           // handed back
    } plan;
    struct { std::vector<kg_iqd_row> rows; std::vector<int32_t> blk_rx, blk_blk, sent; int n, nblk; } last;   // kg_rxbank_iqd_map, _iqd_status
};

// Loran-C (extensions/Loran_C/loran_c.cpp; kg_lorc); its first call also grows the arena slots by its table.  While a receiver is
// started and not in NBFM, its CFastFIR output of the step feeds it in place: ONE launch per step over all such receivers, on the
// tail stream where the IQ display's launch sits.
struct bank_lo {
    kg_lorc *obj;
    kg_dbuf<unsigned char> d_rows; size_t cap; int max_rows;          // the step's rows, each at a multiple of 16 bytes
    std::vector<char> on;                               // `SET start` (the IQ display's registration: one of the two at most)
    struct {
        std::vector<int32_t> list, nblk, row;           // the entries: receiver, blocks, the receiver's row of d_firo
        std::vector<kg_lorc_row> rows; int32_t n;       // handed back
    } plan;
    struct { std::vector<kg_lorc_row> rows; int n; } last;            // kg_rxbank_lorc_map
};

// FAX (extensions/FAX/FaxDecoder.cpp; kg_fax); its first call also grows the arena slots by its table.  While a receiver is started
// and its blocks go on the mono list (the branch in which the reference advances real_wr_pos, rx_sound.cpp:701-703, :1103: not IQ,
// SAS or QAM), the step's d_s16 blocks feed it in place: ONE launch per step over all such receivers, on the tail stream behind
// kg_post_process_dev and ahead of ev_tail.  The counts are the device's.
struct bank_fa {
    kg_fax *obj;
    kg_dbuf<unsigned char> d_rows; size_t row_stride; int max_lines;  // [entry][max_lines][row_stride]
    kg_dbuf<kg_fax_rec> d_recs;                                       // [entry][max_lines]
    kg_dbuf<int32_t> d_counts;                                        // [entry][4]
    std::vector<char> on;                               // `SET fax_start` (ext_register_receive_real_samps_task: the OTHER tap)
    std::vector<double> rate;                           // what ext_update_get_sample_rateHz answers: kg_rxbank_fax_start's srate
    struct {
        // the entries: receiver, blocks, where the receiver's row of d_s16 begins, its sample rate
        std::vector<int32_t> list, nblk; std::vector<int64_t> off; std::vector<double> rate;
    } plan;
    struct { std::vector<int32_t> rx; int n; } last;    // kg_rxbank_fax_out: the last step's entries and their receivers
};

// The CW decoder (extensions/CW_decoder/uhsdr_cw_decoder.cpp; kg_cw); its first call also grows the arena slots by its table.  It is
// the second consumer of the real-samples task tap, fed exactly as FAX is: while a receiver is started and its blocks go on the mono
// list, the step's d_s16 blocks feed it in place: ONE launch per step over all such receivers, on the tail stream behind FAX's and
// ahead of ev_tail.  The counts are the device's; now is what timer_sec() answers during the step (kg_rxbank_cw_set_now).
struct bank_cw {
    kg_cw *obj;
    kg_dbuf<kg_cw_ev> d_evs; int max_events;                          // [entry][max_events]
    kg_dbuf<int32_t> d_counts;                                        // [entry][4]
    std::vector<char> on;                               // `SET cw_start` (ext_register_receive_real_samps_task: one task per receiver)
    uint32_t now;
    struct {
        // the entries: receiver, blocks, where the receiver's row of d_s16 begins, the step's clock
        std::vector<int32_t> list, nblk; std::vector<int64_t> off; std::vector<uint32_t> now;
    } plan;
    struct { std::vector<int32_t> rx; int n; } last;    // kg_rxbank_cw_out: the last step's entries and their receivers
};

// WSPR, stage 1 (extensions/wspr/; kg_wspr); its first call also grows the arena slots by its table.  The third consumer of the IQ tap
// (ext_register_receive_iq_samps, wspr_main.cpp:891): while a receiver captures and is not in NBFM, its CFastFIR output of the step feeds it
// in place, exactly as the IQ display and Loran-C are fed: ONE launch per step over all such receivers, and the cycle-end launch behind it
// when a receiver completes group 85, on the tail stream ahead of ev_tail.  Every block of a step carries the minute and second of the
// last kg_rxbank_wspr_set_now.  Rows, cycles and counts are the device's; the row map and the events are the host's schedule.
struct bank_ws {
    kg_wspr *obj;
    kg_dbuf<unsigned char> d_rows; size_t cap; int max_rows, max_events;   // the step's rows at multiples of KG_WSPR_ROW_STRIDE, in list order
    kg_dbuf<kg_wspr_cycle> d_cycles;                                       // [entry]
    kg_dbuf<int32_t> d_counts;                                             // [entry][4]
    std::vector<char> on;                               // `SET capture=1` (ext_register_receive_iq_samps: one of the three at most)
    int32_t min, sec;
    struct {
        std::vector<int32_t> list, nblk, row, min, sec; // the entries: receiver, blocks, the receiver's row of d_firo; the clock of every block
        std::vector<kg_wspr_row> rows; std::vector<kg_wspr_ev> evs; int32_t n, ne;      // handed back
    } plan;
    struct { std::vector<kg_wspr_row> rows; std::vector<kg_wspr_ev> evs; std::vector<int32_t> rx; int n, ne, nent; } last;      // kg_rxbank_wspr_out
};

// FT8 / FT4, stage 1 (extensions/FT8/; kg_ft8); its first call also grows the arena slots by its table.  The third holder of the
// real-samples task tap (ext_register_receive_real_samps_task, FT8.cpp), fed exactly as FAX and the CW decoder are: while a receiver is
// started and its blocks go on the mono list, the step's d_s16 blocks feed it in place -- a callback a sound block --: the copy, tail
// and monitor launches of the step and, when a receiver's slot ends, sync scores, selection and likelihoods behind them with no host
// wait, on the tail stream behind WSPR's and ahead of ev_tail.  Every callback of a step carries the clock reading of the last
// kg_rxbank_ft8_set_now.  The slot records are the device's; the events and which receiver a record belongs to are the host's schedule.
struct bank_f8 {
    kg_ft8 *obj;
    kg_dbuf<kg_ft8_slot> d_slots;                                          // [nrx]: record k is the k-th receiver of the step whose slot ended
    int max_events;
    std::vector<char> on;                               // kg_rxbank_ft8_start (ext_register_receive_real_samps_task: one task per receiver)
    double now;
    struct {
        std::vector<int32_t> list, nblk; std::vector<int64_t> off; std::vector<double> now;        // the entries: receiver, blocks, its row of d_s16; the clock of every block
        std::vector<kg_ft8_ev> evs; std::vector<int32_t> slot_rx; int32_t ne, nsl;                  // handed back
    } plan;
    struct { std::vector<kg_ft8_ev> evs; std::vector<int32_t> slot_rx; int ne, nsl; } last;        // kg_rxbank_ft8_out
};

struct kg_rxbank {
    // configuration
    int device, nrx, mode, decim_rx;
    size_t n;                                   // ADC samples per step
    size_t blocks_max;                          // sound blocks a receiver can complete in one step
    float rescale, dc_i, dc_q; int spectral_inversion;      // snd_service() unpack, rx/data_pump.cpp:73-74,145-208
    // streams, contexts, the per-seam objects
    hipStream_t s_main, s_side, s_tail, s_up;   // waterfall chain / audio chain / both sequential coders / the table upload
    hipStream_t s_ddc_side;                         // the waterfall DDC's second stream (R = 1 bypass, pass B of R <= 8 beside the rest)
    kg_ctx *c_main, *c_side, *c_tail;
    kg_ddc *ddc; kg_wf *wf; kg_rxddc *rx; kg_fir *fir; kg_post *post; kg_adpcm *adpcm;
    kg_nb *nb;                                  // m_NoiseProc_snd[] (the waterfall's blankers are kg_wf's)
    kg_fir *nullfir;                            // m_chan_null_FIR[] (rx_sound.cpp:151), on the tail stream behind kg_post
    bank_fx fx; bank_iq iq; bank_lo lo; bank_fa fa; bank_cw cw; bank_ws ws; bank_f8 f8;     // the extensions (above)
    // device buffers
    kg_dbuf<short2> d_wfiq; size_t wf_stride;         // [nrx][wf_stride] iq_t: a one-shot receiver uses pairs 0 .. 8191 of its row, an overlapped one all of it
    kg_dbuf<unsigned char> d_rows, d_pkts;         // [frame][1024], [frame][BANK_PKT_STRIDE]
    kg_dbuf<unsigned char> d_raw; size_t nrec_max;     // [nrx][nrec_max] rx_iq_t (6 bytes)
    kg_dbuf<float2> d_xin, d_firo; size_t firo_stride; // [nrx][nrec_max], [nrx][firo_stride]
    kg_dbuf<short> d_s16; kg_dbuf<unsigned char> d_pay; // [nrx][firo_stride], [nrx][firo_stride / 2]
    kg_dbuf<float2> d_agc; kg_dbuf<unsigned char> d_iqpay; // [nrx][firo_stride] the AGC's complex output, [nrx][4 firo_stride] the IQ mode's payload
    kg_dbuf<unsigned char> d_spec; size_t spec_max;     // [spec_max][1024] u8: the step's rows in map order
    // the receivers, and the step being made
    std::vector<bank_rx> rcv;
    bank_plan plan;
    // the last step's maps (kg_rxbank_spec_map, _frame_map) and info
    int spec_n;
    std::vector<int32_t> spec_rx, spec_inst, spec_blk, frame_rx, pkt_bytes;
    std::vector<uint64_t> frame_off;
    kg_rxbank_step_info last;
    // step tables: BANK_SLOTS pinned host / device slots
    kg_arena arena; kg_hbuf<unsigned char> h_slots; kg_dbuf<unsigned char> d_slots; size_t slot_bytes;
    hipEvent_t ev_end[BANK_SLOTS][3];           // behind a step's last enqueue on main / side / tail
    bool ev_end_rec[BANK_SLOTS];
    hipEvent_t ev_tab, ev_fir, ev_tail, ev_frames, ev_pk;
    bool tail_pending, pk_pending;
    uint64_t step;
    // where the host's share of a step goes (kg_rxbank_host_profile): seconds per phase, summed over `prof_steps` steps
    double prof[16]; uint64_t prof_steps;
};

enum { PF_PLAN = 0, PF_UPLOAD, PF_RXDDC, PF_UNPACK, PF_FIR, PF_POST, PF_ADPCM, PF_DDC, PF_FRAMES, PF_PKT, PF_EVENTS, PF_END, PF_N };
static const char *const PF_NAME[PF_N] = {"plan pass", "slot wait + upload", "rxddc", "unpack", "fir", "post", "adpcm", "wf ddc", "frames", "packets",
                                          "events between the chains", "end-of-step events"};
struct bank_tick {
    std::chrono::steady_clock::time_point t;
    bank_tick() : t(std::chrono::steady_clock::now()) {}
    void lap(kg_rxbank *b, int k, bool on) {
        const auto n = std::chrono::steady_clock::now();
        if (on) b->prof[k] += std::chrono::duration<double>(n - t).count();
        t = n;
    }
};

// The streams of closed banks are kept for the next one (per device, never destroyed).  Which hardware queue a NEW stream lands
// on is the HIP runtime's choice at that moment, and a process that had created and destroyed a few banks got streams whose
// kernels took turns instead of running side by side: every later bank of the default bench run stepped in 1.37 ... 1.50 ms
// where the first one took 1.24 (and the same bank 0.98 alone).  A bank that inherits the streams of the first keeps its
// placement.
struct bank_stream_set { int device; hipStream_t s[5]; };
static std::vector<bank_stream_set> g_free_sets;
static std::mutex g_free_mutex;

static void bank_set_arena(kg_rxbank *b, int mode)
{
    b->arena.mode = mode;
    kg_arena *a = mode == KG_ARENA_OFF ? nullptr : &b->arena;
    b->c_main->arena = a; b->c_side->arena = a; b->c_tail->arena = a;
}

static int bank_rx_check(kg_rxbank *b, int rx, const char *who)
{
    KG_REQUIRE(b != nullptr, KG_ERR_INVALID, "%s: null argument", who);
    KG_REQUIRE(rx >= 0 && rx < b->nrx, KG_ERR_INVALID, "%s: receiver %d (0..%d)", who, rx, b->nrx - 1);
    return KG_OK;
}

// the host waits for everything the bank has enqueued (with_upload: the table upload's stream too)
static int bank_drain(kg_rxbank *b, bool with_upload)
{
    if (with_upload) KG_HIP(hipStreamSynchronize(b->s_up));
    for (hipStream_t s : {b->s_main, b->s_side, b->s_tail}) KG_HIP(hipStreamSynchronize(s));
    return KG_OK;
}

// IS_STEREO (IQ, SAS, QAM): the blocks that go out as (s2_t) pairs and never onto the mono list
static bool bank_stereo(int mode) { return mode == KG_POST_IQ || mode == KG_POST_SAS || mode == KG_POST_QAM; }

// ---- the extensions' functions, the same set for each record:
//   _sizes       at create: what the bank can hold for it, the host lists' capacity (a step allocates nothing)
//   _ensure      the first call that names it: object and buffers, through bank_ext_ensure
//   _fresh       a connection's end or beginning on one receiver
//   _plan_clear, _plan    the step's lists: emptied, then entry i of the active list (receiver p.act[i], nblk sound blocks)
//   _enqueue     its ONE launch of the step, on the tail stream; what the entry point hands back goes into the record's plan
//   _commit      the plan's maps become the last step's
// The general functions call the six by name, in the order fx, iq, lo, fa, cw, ws, f8: that is the order of the launches on the tail stream
// and of the tables in the slot.

// A device buffer of a record: where its pointer goes, its size, its name in a refusal
struct bank_want { void **p; size_t bytes; const char *what; };
template <class T> static bank_want bank_buf(kg_dbuf<T> &d, size_t count, const char *what) { return bank_want{(void **) &d.p, sizeof(T) * count, what}; }

// An extension's first use, made whole or not at all: the buffers zeroed, the arena slots grown by `table` bytes (0: as they are;
// the growth is cumulative: slot_bytes + table, rounded to 64, BANK_SLOTS of them pinned and on the device), then `make`, which
// creates the object and stores it in its record as its last act.  Everything is allocated into locals and changes hands by swap once
// nothing can fail any more.  Drains the bank's streams, the upload's included: no step is in flight while the slots change.
static int bank_ext_ensure(kg_rxbank *b, const char *who, std::initializer_list<bank_want> bufs, size_t table, int (*make)(kg_rxbank *))
{
    KG_HIP(hipSetDevice(b->device));
    KG_TRY(bank_drain(b, true));
    char slots[64];
    snprintf(slots, sizeof slots, "%s: slots", who);
    kg_hbuf<unsigned char> h;
    kg_dbuf<unsigned char> d;
    std::vector<kg_dbuf<unsigned char>> got(bufs.size());
    const size_t grown = (b->slot_bytes + table + 63) & ~(size_t) 63;
    if (table) {
        KG_TRY(h.alloc(grown * BANK_SLOTS, slots));
        KG_TRY(d.alloc(grown * BANK_SLOTS, slots));
    }
    size_t n = 0;
    for (const bank_want &w : bufs) {
        KG_TRY(got[n].alloc(w.bytes, w.what));
        if (hipMemset(got[n++], 0, w.bytes) != hipSuccess) { kg_set_error("%s: hipMemset failed", who); return KG_ERR_HIP; }
    }
    KG_TRY(make(b));
    n = 0;
    for (const bank_want &w : bufs) { void *old = *w.p; *w.p = got[n].p; got[n++].p = (unsigned char *) old; }
    if (table) { std::swap(b->h_slots.p, h.p); std::swap(b->d_slots.p, d.p); b->slot_bytes = grown; }      // the old slots go with h and d
    return KG_OK;
}

static void bank_fx_sizes(kg_rxbank *b)
{
    bank_fx &x = b->fx;
    x.stride = b->blocks_max * KG_FFTEXT_ROW; x.max = b->blocks_max * (size_t) b->nrx;        // a receiver's function takes ONE instance's blocks
    x.on.assign((size_t) b->nrx, 0);
    for (std::vector<int32_t> *v : {&x.plan.list, &x.plan.nblk, &x.plan.inst, &x.plan.row, &x.plan.blk0}) v->reserve(2 * x.max);
    x.plan.nullpos.assign(b->blocks_max, 0);
}

static int bank_fx_ensure(kg_rxbank *b)
{
    bank_fx &x = b->fx;
    if (x.obj) return KG_OK;
    KG_TRY(bank_ext_ensure(b, "kg_rxbank_fftext",
                           {bank_buf(x.d_post, 2 * (size_t) b->nrx * x.stride, "kg_rxbank_fftext: spectra"),
                            bank_buf(x.d_rows, x.max * KG_FFTEXT_ROW, "kg_rxbank_fftext: rows")},
                           0, [](kg_rxbank *b) {           // a rate set before the first use goes to the new object
                               kg_fftext *fx = nullptr;
                               int rc = kg_fftext_create(b->c_tail, b->nrx, &fx);
                               if (rc == KG_OK && b->fx.rate > 0) rc = kg_fftext_set_rate(fx, b->fx.rate);
                               if (rc == KG_OK) b->fx.obj = fx; else kg_fftext_destroy(fx);
                               return rc;
                           }));
    for (std::vector<int32_t> *v : {&x.last.rx, &x.last.blk, &x.last.bin, &x.plan.rx, &x.plan.blk, &x.plan.bin, &x.plan.ent}) v->assign(x.max, 0);
    return KG_OK;
}

// ext_unregister_receive_FFT_samps at the connection's end, its fft_t gone with it; a new one's: function off, nothing latched, sums zero
static int bank_fx_fresh(kg_rxbank *b, int rx) { b->fx.on[rx] = 0; return b->fx.obj ? kg_fftext_restart(b->fx.obj, rx) : KG_OK; }

static void bank_fx_plan_clear(kg_rxbank *b)
{
    bank_fx &x = b->fx;
    for (std::vector<int32_t> *v : {&x.plan.list, &x.plan.nblk, &x.plan.inst, &x.plan.row, &x.plan.blk0}) v->clear();
    std::fill(x.plan.nullpos.begin(), x.plan.nullpos.end(), 0);
    x.plan.n = 0;
}

static void bank_fx_plan(kg_rxbank *b, int i, int nblk)
{
    bank_fx &x = b->fx;
    const bank_plan &p = b->plan;
    if (!x.obj) return;
    const int k = p.act[i], NR = b->nrx;
    auto put = [&x, k](int n, int inst, size_t row, int blk0) {
        x.plan.list.push_back(k); x.plan.nblk.push_back(n); x.plan.inst.push_back(inst); x.plan.row.push_back((int32_t) row); x.plan.blk0.push_back(blk0);
    };
    if (x.on[k] && nblk > 0) put(nblk, KG_SPEC_PASSBAND, (size_t) i * b->blocks_max, 0);      // each filter hands every block of its own to fft_data, which takes one instance's
    if (p.sam_null[i])                                     // where sound block blk's channel-null call leaves this receiver's spectrum
        for (int blk = 0; blk < nblk; blk++) {
            const int pos = x.plan.nullpos[blk]++;
            if (x.on[k]) put(1, KG_SPEC_CHAN_NULL, (size_t) NR * b->blocks_max + (size_t) blk * NR + pos, blk);
        }
}

// fft_data over the step's blocks: one launch, behind both filters
static int bank_fx_enqueue(kg_rxbank *b)
{
    bank_fx &x = b->fx;
    if (x.plan.list.empty()) return KG_OK;
    const int rc = kg_fftext_process_rows_(x.obj, x.plan.list.data(), (int) x.plan.list.size(), x.plan.nblk.data(), x.plan.inst.data(), x.plan.row.data(),
                                           (const float *) x.d_post.p, KG_FFTEXT_ROW, x.d_rows, KG_FFTEXT_ROW, (int) x.max, x.plan.rx.data(), x.plan.ent.data(),
                                           x.plan.blk.data(), x.plan.bin.data());
    if (rc < 0) return rc;
    x.plan.n = rc;
    return KG_OK;
}

static void bank_fx_commit(kg_rxbank *b)
{
    bank_fx &x = b->fx;
    for (int r = 0; r < x.plan.n; r++) x.plan.blk[r] += x.plan.blk0[x.plan.ent[r]];       // the sound block of the step
    x.last.n = x.plan.n;
    x.last.rx.swap(x.plan.rx); x.last.blk.swap(x.plan.blk); x.last.bin.swap(x.plan.bin);
}

static void bank_iq_sizes(kg_rxbank *b)
{
    bank_iq &x = b->iq;
    const size_t nrx = (size_t) b->nrx;
    x.cap = nrx * (KG_FIR_OUT * b->blocks_max + KG_IQD_RING) * 4;
    // a row per sample at points = 1; the map is the host's, so a large bank's is bounded (a step with more rows is refused)
    const size_t rows = nrx * b->blocks_max * KG_FIR_OUT;
    x.max_rows = (int) (rows < ((size_t) 1 << 18) ? rows : ((size_t) 1 << 18));
    x.on.assign(nrx, 0);
    for (std::vector<int32_t> *v : {&x.plan.list, &x.plan.nblk, &x.plan.inst, &x.plan.row}) v->reserve(nrx);
}

static int bank_iq_ensure(kg_rxbank *b)
{
    bank_iq &x = b->iq;
    if (x.obj) return KG_OK;
    const size_t nst = (size_t) b->nrx * b->blocks_max;
    KG_TRY(bank_ext_ensure(b, "kg_rxbank_iqd", {bank_buf(x.d_rows, x.cap, "kg_rxbank_iqd: rows"), bank_buf(x.d_st, nst, "kg_rxbank_iqd: status")}, 0,
                           [](kg_rxbank *b) { return kg_iqd_create(b->c_tail, b->nrx, &b->iq.obj); }));
    for (std::vector<kg_iqd_row> *v : {&x.last.rows, &x.plan.rows}) v->assign((size_t) x.max_rows, kg_iqd_row{});
    for (std::vector<int32_t> *v : {&x.last.sent, &x.plan.sent, &x.last.blk_rx, &x.last.blk_blk}) v->assign(nst, 0);
    return KG_OK;
}

// iq_display_close: the object goes with the connection; a new connection's is a fresh one, not registered
static int bank_iq_fresh(kg_rxbank *b, int rx) { b->iq.on[rx] = 0; return b->iq.obj ? kg_iqd_init(b->iq.obj, rx) : KG_OK; }

static void bank_iq_plan_clear(kg_rxbank *b)
{
    bank_iq &x = b->iq;
    for (std::vector<int32_t> *v : {&x.plan.list, &x.plan.nblk, &x.plan.inst, &x.plan.row}) v->clear();
    x.plan.n = 0;
}

static void bank_iq_plan(kg_rxbank *b, int i, int nblk)
{
    bank_iq &x = b->iq;
    const int k = b->plan.act[i];
    if (!x.obj || !x.on[k] || nblk <= 0 || b->plan.mode[i] == KG_POST_NBFM) return;       // receive_iq_pre_agc is NULL while isNBFM (rx_sound.cpp:492)
    x.plan.list.push_back(k); x.plan.nblk.push_back(nblk); x.plan.inst.push_back(0); x.plan.row.push_back(k);
}

// iq_display_data over the step's blocks: one launch, behind the filter, ahead of ev_tail
static int bank_iq_enqueue(kg_rxbank *b)
{
    bank_iq &x = b->iq;
    if (x.plan.list.empty()) return KG_OK;
    const int rc = kg_iqd_process_rows_(x.obj, x.plan.list.data(), (int) x.plan.list.size(), x.plan.nblk.data(), x.plan.inst.data(), x.plan.row.data(), KG_FIR_OUT,
                                        (const float *) b->d_firo.p, b->firo_stride, x.d_rows, x.cap, x.d_st, (size_t) b->nrx * b->blocks_max,
                                        x.plan.rows.data(), x.max_rows, x.plan.sent.data());
    if (rc < 0) return rc;
    x.plan.n = rc;
    return KG_OK;
}

static void bank_iq_commit(kg_rxbank *b)
{
    bank_iq &x = b->iq;
    x.last.n = x.plan.n; x.last.nblk = 0;
    if (!x.obj) return;
    x.last.rows.swap(x.plan.rows); x.last.sent.swap(x.plan.sent);
    for (size_t e = 0; e < x.plan.list.size(); e++)
        for (int blk = 0; blk < x.plan.nblk[e]; blk++) { x.last.blk_rx[x.last.nblk] = x.plan.list[e]; x.last.blk_blk[x.last.nblk] = blk; x.last.nblk++; }
}

static void bank_lo_sizes(kg_rxbank *b)
{
    bank_lo &x = b->lo;
    const size_t nrx = (size_t) b->nrx;
    // a row per run at most: BANK_LO_RUNS rows of up to 1200 bytes per receiver and Loran channel
    x.max_rows = (int) (nrx * 2 * BANK_LO_RUNS(b->blocks_max));
    x.cap = (size_t) x.max_rows * 1200;
    x.on.assign(nrx, 0);
    for (std::vector<int32_t> *v : {&x.plan.list, &x.plan.nblk, &x.plan.row}) v->reserve(nrx);
}

static int bank_lo_ensure(kg_rxbank *b)
{
    bank_lo &x = b->lo;
    if (x.obj) return KG_OK;
    KG_TRY(bank_ext_ensure(b, "kg_rxbank_lorc", {bank_buf(x.d_rows, x.cap, "kg_rxbank_lorc: rows")},
                           kg_lorc_table_bytes_((size_t) b->nrx, BANK_LO_RUNS(b->blocks_max)),
                           [](kg_rxbank *b) { return kg_lorc_create(b->c_tail, b->nrx, &b->lo.obj); }));
    for (std::vector<kg_lorc_row> *v : {&x.last.rows, &x.plan.rows}) v->assign((size_t) x.max_rows, kg_lorc_row{});
    return KG_OK;
}

// the connection's end or beginning: loran_c[rx] as a new connection finds it -- stopped, waiting for its `SET ext_server_init`
static int bank_lo_fresh(kg_rxbank *b, int rx) { b->lo.on[rx] = 0; return b->lo.obj ? kg_lorc_reset_(b->lo.obj, rx) : KG_OK; }

static void bank_lo_plan_clear(kg_rxbank *b) { b->lo.plan.list.clear(); b->lo.plan.nblk.clear(); b->lo.plan.row.clear(); b->lo.plan.n = 0; }

static void bank_lo_plan(kg_rxbank *b, int i, int nblk)
{
    bank_lo &x = b->lo;
    const int k = b->plan.act[i];
    if (!x.obj || !x.on[k] || nblk <= 0 || b->plan.mode[i] == KG_POST_NBFM) return;       // the IQ display's tap, and its NBFM rule
    x.plan.list.push_back(k); x.plan.nblk.push_back(nblk); x.plan.row.push_back(k);
}

// loran_c_data over the step's blocks: one launch, reading d_firo in place
static int bank_lo_enqueue(kg_rxbank *b)
{
    bank_lo &x = b->lo;
    if (x.plan.list.empty()) return KG_OK;
    return kg_lorc_process_rows_(x.obj, x.plan.list.data(), (int) x.plan.list.size(), x.plan.nblk.data(), x.plan.row.data(), KG_FIR_OUT, (const float *) b->d_firo.p,
                                 b->firo_stride, x.d_rows, x.cap, x.plan.rows.data(), x.max_rows, &x.plan.n);
}

static void bank_lo_commit(kg_rxbank *b) { b->lo.last.n = b->lo.plan.n; if (b->lo.obj) b->lo.last.rows.swap(b->lo.plan.rows); }

static void bank_fa_sizes(kg_rxbank *b)
{
    bank_fa &x = b->fa;
    const size_t nrx = (size_t) b->nrx;
    x.max_lines = (int) ((b->blocks_max * (2 * KG_FAX_BLK + 2) + BANK_FAX_MIN_SPL - 1) / BANK_FAX_MIN_SPL) + 1;
    x.row_stride = (BANK_FAX_MAX_WIDTH + 1 + 15) & ~(size_t) 15;
    x.on.assign(nrx, 0); x.rate.assign(nrx, 0.0);
    for (std::vector<int32_t> *v : {&x.plan.list, &x.plan.nblk}) v->reserve(nrx);
    x.plan.off.reserve(nrx); x.plan.rate.reserve(nrx);
    x.last.rx.assign(nrx, -1);
}

static int bank_fa_ensure(kg_rxbank *b)
{
    bank_fa &x = b->fa;
    if (x.obj) return KG_OK;
    const size_t nrows = (size_t) b->nrx * (size_t) x.max_lines;
    return bank_ext_ensure(b, "kg_rxbank_fax",
                           {bank_buf(x.d_rows, nrows * x.row_stride, "kg_rxbank_fax: rows"), bank_buf(x.d_recs, nrows, "kg_rxbank_fax: records"),
                            bank_buf(x.d_counts, (size_t) 4 * b->nrx, "kg_rxbank_fax: counts")},
                           kg_fax_table_bytes_((size_t) b->nrx), [](kg_rxbank *b) { return kg_fax_create(b->c_tail, b->nrx, &b->fa.obj); });
}

// the connection's end or beginning: m_FaxDecoder[rx] and fax[rx] as a new connection finds them -- zeroed, no task
static int bank_fa_fresh(kg_rxbank *b, int rx) { b->fa.on[rx] = 0; b->fa.rate[rx] = 0; return b->fa.obj ? kg_fax_reset_(b->fa.obj, rx) : KG_OK; }

static void bank_fa_plan_clear(kg_rxbank *b) { b->fa.plan.list.clear(); b->fa.plan.nblk.clear(); b->fa.plan.off.clear(); b->fa.plan.rate.clear(); }

static void bank_fa_plan(kg_rxbank *b, int i, int nblk)
{
    bank_fa &x = b->fa;
    const int k = b->plan.act[i];
    if (!x.obj || !x.on[k] || nblk <= 0 || bank_stereo(b->plan.mode[i])) return;      // real_wr_pos advances for the mono blocks alone: fax_task sees no other
    x.plan.list.push_back(k); x.plan.nblk.push_back(nblk); x.plan.off.push_back((int64_t) ((size_t) k * b->firo_stride)); x.plan.rate.push_back(x.rate[k]);
}

// ProcessSamples over the step's blocks: one launch, reading d_s16 in place
static int bank_fa_enqueue(kg_rxbank *b)
{
    bank_fa &x = b->fa;
    if (x.plan.list.empty()) return KG_OK;
    return kg_fax_push_at_(x.obj, x.plan.list.data(), (int) x.plan.list.size(), x.plan.nblk.data(), x.plan.off.data(), (const int16_t *) b->d_s16.p, b->firo_stride,
                           x.plan.rate.data(), x.d_rows, x.row_stride, x.d_recs, x.max_lines, x.d_counts);
}

static void bank_fa_commit(kg_rxbank *b)
{
    bank_fa &x = b->fa;
    x.last.n = (int) x.plan.list.size();
    for (int e = 0; e < x.last.n; e++) x.last.rx[e] = x.plan.list[e];
}

static void bank_cw_sizes(kg_rxbank *b)
{
    bank_cw &x = b->cw;
    const size_t nrx = (size_t) b->nrx;
    x.max_events = KG_CW_EVENTS_PER_GBLK * (int) ((b->blocks_max * KG_CW_BLK + KG_CW_GBLK - 1) / KG_CW_GBLK);       // kg_cw_max_events' rule
    x.on.assign(nrx, 0);
    x.now = 0;
    for (std::vector<int32_t> *v : {&x.plan.list, &x.plan.nblk}) v->reserve(nrx);
    x.plan.off.reserve(nrx); x.plan.now.reserve(nrx);
    x.last.rx.assign(nrx, -1);
}

static int bank_cw_ensure(kg_rxbank *b)
{
    bank_cw &x = b->cw;
    if (x.obj) return KG_OK;
    KG_REQUIRE(kg_cw_max_events((int) b->blocks_max) >= 0, KG_ERR_INVALID, "kg_rxbank_cw: a step of up to %zu sound blocks a receiver; a push takes 256", b->blocks_max);
    return bank_ext_ensure(b, "kg_rxbank_cw",
                           {bank_buf(x.d_evs, (size_t) b->nrx * (size_t) x.max_events, "kg_rxbank_cw: events"),
                            bank_buf(x.d_counts, (size_t) 4 * b->nrx, "kg_rxbank_cw: counts")},
                           kg_cw_table_bytes_((size_t) b->nrx), [](kg_rxbank *b) { return kg_cw_create(b->c_tail, b->nrx, &b->cw.obj); });
}

// the connection's end or beginning: cw_decoder[rx] as a new connection finds it -- zeroed, no task
static int bank_cw_fresh(kg_rxbank *b, int rx) { b->cw.on[rx] = 0; return b->cw.obj ? kg_cw_reset_(b->cw.obj, rx) : KG_OK; }

static void bank_cw_plan_clear(kg_rxbank *b) { b->cw.plan.list.clear(); b->cw.plan.nblk.clear(); b->cw.plan.off.clear(); b->cw.plan.now.clear(); }

static void bank_cw_plan(kg_rxbank *b, int i, int nblk)
{
    bank_cw &x = b->cw;
    const int k = b->plan.act[i];
    if (!x.obj || !x.on[k] || nblk <= 0 || bank_stereo(b->plan.mode[i])) return;      // real_wr_pos advances for the mono blocks alone: cw_task sees no other
    x.plan.list.push_back(k); x.plan.nblk.push_back(nblk); x.plan.off.push_back((int64_t) ((size_t) k * b->firo_stride)); x.plan.now.push_back(x.now);
}

// CwDecode_RxProcessor over the step's blocks: one launch, reading d_s16 in place
static int bank_cw_enqueue(kg_rxbank *b)
{
    bank_cw &x = b->cw;
    if (x.plan.list.empty()) return KG_OK;
    return kg_cw_push_at_(x.obj, x.plan.list.data(), (int) x.plan.list.size(), x.plan.nblk.data(), x.plan.off.data(), (const int16_t *) b->d_s16.p, b->firo_stride,
                          x.plan.now.data(), x.d_evs, x.max_events, x.d_counts);
}

static void bank_cw_commit(kg_rxbank *b)
{
    bank_cw &x = b->cw;
    x.last.n = (int) x.plan.list.size();
    for (int e = 0; e < x.last.n; e++) x.last.rx[e] = x.plan.list[e];
}

#define BANK_WS_OPS(blocks_) (4 * (size_t) (blocks_) + 4)      /* a callback of 512 samples: a clear, two copy runs and a group at most */

static void bank_ws_sizes(kg_rxbank *b)
{
    bank_ws &x = b->ws;
    const size_t nrx = (size_t) b->nrx;
    x.max_rows = (int) (nrx * (b->blocks_max + 1));     // a group a callback at most (int_decimate >= 1)
    x.cap = (size_t) x.max_rows * KG_WSPR_ROW_STRIDE;
    x.max_events = (int) (nrx * 16);                    // 8 pending, the sync, DECODING / PEAKS / resume of the one cycle end a step can hold
    x.on.assign(nrx, 0);
    x.min = x.sec = 0;
    for (std::vector<int32_t> *v : {&x.plan.list, &x.plan.nblk, &x.plan.row}) v->reserve(nrx);
    for (std::vector<int32_t> *v : {&x.plan.min, &x.plan.sec}) v->reserve(nrx * b->blocks_max);
    x.last.rx.assign(nrx, -1);
}

static int bank_ws_ensure(kg_rxbank *b)
{
    bank_ws &x = b->ws;
    if (x.obj) return KG_OK;
    KG_TRY(bank_ext_ensure(b, "kg_rxbank_wspr",
                           {bank_buf(x.d_rows, x.cap, "kg_rxbank_wspr: rows"), bank_buf(x.d_cycles, (size_t) b->nrx, "kg_rxbank_wspr: cycles"),
                            bank_buf(x.d_counts, (size_t) 4 * b->nrx, "kg_rxbank_wspr: counts")},
                           kg_wspr_table_bytes_((size_t) b->nrx, BANK_WS_OPS(b->blocks_max)), [](kg_rxbank *b) { return kg_wspr_create(b->c_tail, b->nrx, &b->ws.obj); }));
    for (std::vector<kg_wspr_row> *v : {&x.last.rows, &x.plan.rows}) v->assign((size_t) x.max_rows, kg_wspr_row{});
    for (std::vector<kg_wspr_ev> *v : {&x.last.evs, &x.plan.evs}) v->assign((size_t) x.max_events, kg_wspr_ev{});
    return KG_OK;
}

// the connection's end or beginning: wspr[rx] as a new connection finds it -- zeroed, not capturing, waiting for its `SET ext_server_init`
static int bank_ws_fresh(kg_rxbank *b, int rx) { b->ws.on[rx] = 0; return b->ws.obj ? kg_wspr_reset_(b->ws.obj, rx) : KG_OK; }

static void bank_ws_plan_clear(kg_rxbank *b)
{
    bank_ws &x = b->ws;
    for (std::vector<int32_t> *v : {&x.plan.list, &x.plan.nblk, &x.plan.row, &x.plan.min, &x.plan.sec}) v->clear();
    x.plan.n = x.plan.ne = 0;
}

static void bank_ws_plan(kg_rxbank *b, int i, int nblk)
{
    bank_ws &x = b->ws;
    const int k = b->plan.act[i];
    if (!x.obj || !x.on[k] || nblk <= 0 || b->plan.mode[i] == KG_POST_NBFM) return;       // the IQ display's tap, and its NBFM rule
    x.plan.list.push_back(k); x.plan.nblk.push_back(nblk); x.plan.row.push_back(k);
    x.plan.min.insert(x.plan.min.end(), b->blocks_max, x.min); x.plan.sec.insert(x.plan.sec.end(), b->blocks_max, x.sec);
}

// wspr_data over the step's blocks: one launch, reading d_firo in place, and the cycle-end launch when one is due
static int bank_ws_enqueue(kg_rxbank *b)
{
    bank_ws &x = b->ws;
    if (x.plan.list.empty()) return KG_OK;
    return kg_wspr_push_rows_(x.obj, x.plan.list.data(), (int) x.plan.list.size(), x.plan.nblk.data(), x.plan.row.data(), KG_FIR_OUT, (const float *) b->d_firo.p,
                              b->firo_stride, x.plan.min.data(), x.plan.sec.data(), b->blocks_max, x.d_rows, x.cap, x.plan.rows.data(), x.max_rows, &x.plan.n,
                              x.plan.evs.data(), x.max_events, &x.plan.ne, x.d_cycles, x.d_counts);
}

static void bank_ws_commit(kg_rxbank *b)
{
    bank_ws &x = b->ws;
    x.last.n = x.plan.n; x.last.ne = x.plan.ne; x.last.nent = (int) x.plan.list.size();
    if (!x.obj) return;
    x.last.rows.swap(x.plan.rows); x.last.evs.swap(x.plan.evs);
    for (int e = 0; e < x.last.nent; e++) x.last.rx[e] = x.plan.list[e];
}

static void bank_f8_sizes(kg_rxbank *b)
{
    bank_f8 &x = b->f8;
    const size_t nrx = (size_t) b->nrx;
    x.max_events = (int) (nrx * 4);                     // a sync, the one slot end a step can hold, the next sync
    x.on.assign(nrx, 0);
    x.now = 0.0;
    for (std::vector<int32_t> *v : {&x.plan.list, &x.plan.nblk}) v->reserve(nrx);
    x.plan.off.reserve(nrx); x.plan.now.reserve(nrx * b->blocks_max);
    x.plan.ne = x.plan.nsl = x.last.ne = x.last.nsl = 0;
}

static int bank_f8_ensure(kg_rxbank *b)
{
    bank_f8 &x = b->f8;
    if (x.obj) return KG_OK;
    KG_REQUIRE(b->blocks_max <= 4096 && b->blocks_max * KG_FIR_OUT < 85248, KG_ERR_INVALID,
               "kg_rxbank_ft8: a step of up to %zu sound blocks a receiver; a step may hold one slot end (under 166 blocks)", b->blocks_max);
    KG_TRY(bank_ext_ensure(b, "kg_rxbank_ft8", {bank_buf(x.d_slots, (size_t) b->nrx, "kg_rxbank_ft8: slot records")}, kg_ft8_table_bytes_((size_t) b->nrx, b->blocks_max),
                           [](kg_rxbank *b) { return kg_ft8_create(b->c_tail, b->nrx, &b->f8.obj); }));
    for (std::vector<kg_ft8_ev> *v : {&x.last.evs, &x.plan.evs}) v->assign((size_t) x.max_events, kg_ft8_ev{});
    for (std::vector<int32_t> *v : {&x.last.slot_rx, &x.plan.slot_rx}) v->assign((size_t) b->nrx, -1);
    return KG_OK;
}

// the connection's end or beginning: decode_ft8[rx] as a new connection finds it -- not initialised, no task, last_frame zeroed
static int bank_f8_fresh(kg_rxbank *b, int rx) { b->f8.on[rx] = 0; return b->f8.obj ? kg_ft8_reset_(b->f8.obj, rx) : KG_OK; }

static void bank_f8_plan_clear(kg_rxbank *b)
{
    bank_f8 &x = b->f8;
    x.plan.list.clear(); x.plan.nblk.clear(); x.plan.off.clear(); x.plan.now.clear();
    x.plan.ne = x.plan.nsl = 0;
}

static void bank_f8_plan(kg_rxbank *b, int i, int nblk)
{
    bank_f8 &x = b->f8;
    const int k = b->plan.act[i];
    if (!x.obj || !x.on[k] || nblk <= 0 || bank_stereo(b->plan.mode[i])) return;      // real_wr_pos advances for the mono blocks alone
    x.plan.list.push_back(k); x.plan.nblk.push_back(nblk); x.plan.off.push_back((int64_t) ((size_t) k * b->firo_stride));
    x.plan.now.insert(x.plan.now.end(), b->blocks_max, x.now);
}

// decode_ft8_samples over the step's blocks, reading d_s16 in place: the monitor's launches and the slot-end chain when one is due
static int bank_f8_enqueue(kg_rxbank *b)
{
    bank_f8 &x = b->f8;
    if (x.plan.list.empty()) return KG_OK;
    return kg_ft8_push_at_(x.obj, x.plan.list.data(), (int) x.plan.list.size(), x.plan.nblk.data(), x.plan.off.data(), KG_FIR_OUT, (const int16_t *) b->d_s16.p,
                           b->firo_stride, x.plan.now.data(), b->blocks_max, x.plan.evs.data(), x.max_events, &x.plan.ne, x.d_slots, b->nrx, x.plan.slot_rx.data(),
                           &x.plan.nsl);
}

static void bank_f8_commit(kg_rxbank *b)
{
    bank_f8 &x = b->f8;
    x.last.ne = x.plan.ne; x.last.nsl = x.plan.nsl;
    if (!x.obj) return;
    x.last.evs.swap(x.plan.evs); x.last.slot_rx.swap(x.plan.slot_rx);
}

// a connection ends or begins on receiver rx: every extension as a new connection finds it
static int bank_ext_fresh(kg_rxbank *b, int rx)
{
    KG_TRY(bank_fx_fresh(b, rx));
    KG_TRY(bank_iq_fresh(b, rx));
    KG_TRY(bank_lo_fresh(b, rx));
    KG_TRY(bank_fa_fresh(b, rx));
    KG_TRY(bank_cw_fresh(b, rx));
    KG_TRY(bank_ws_fresh(b, rx));
    return bank_f8_fresh(b, rx);
}

// The real-samples task tap (ext_register_receive_real_samps_task) holds one task per receiver, FAX's, the CW decoder's or FT8's: whoever
// asks for it is refused while one of the other two has it
enum { TAP_FAX = 0, TAP_CW = 1, TAP_FT8 = 2 };
static int bank_real_tap_free(const kg_rxbank *b, int rx, const char *who, int asker)
{
    const char *holder = asker != TAP_FT8 && b->f8.on[rx] ? "FT8 started" : asker != TAP_FAX && b->fa.on[rx] ? "FAX started" :
                         asker != TAP_CW && b->cw.on[rx] ? "the CW decoder started" : nullptr;
    KG_REQUIRE(holder == nullptr, KG_ERR_STATE, "%s: receiver %d has %s; the tap holds one task", who, rx, holder);
    return KG_OK;
}

// The IQ tap (ext_users[rx].receive_iq_pre_agc) holds one callback, the IQ display's, Loran-C's or WSPR's: whoever asks for it is refused
// while another has it
static int bank_tap_free(const kg_rxbank *b, int rx, const char *who, bool lorc_asks)
{
    KG_REQUIRE(!b->ws.on[rx], KG_ERR_STATE, "%s: receiver %d has WSPR capturing; the tap holds one callback", who, rx);
    KG_REQUIRE(!(lorc_asks ? b->iq.on[rx] : b->lo.on[rx]), KG_ERR_STATE, "%s: receiver %d has %s; the tap holds one callback", who, rx,
               lorc_asks ? "the IQ display running" : "Loran-C started");
    return KG_OK;
}

static int bank_tap_free_for_wspr(const kg_rxbank *b, int rx, const char *who)
{
    KG_REQUIRE(!b->iq.on[rx] && !b->lo.on[rx], KG_ERR_STATE, "%s: receiver %d has %s; the tap holds one callback", who, rx,
               b->iq.on[rx] ? "the IQ display running" : "Loran-C started");
    return KG_OK;
}

// the prologue of an extension's per-receiver entry point: the receiver exists, the extension is made
#define BANK_EXT(who, ensure)                          \
    KG_TRY(bank_rx_check(b, rx, who));                 \
    KG_TRY(ensure(b))

// ---- plan: what the step is.  No HIP call, no table staged, no bank state written: only b->plan and the records' plan halves.

// Entry i's rows: which of its nblk sound blocks give an audio spectrum row -- the reference's rule (kg_spec.h), walked on a copy of
// the mirror that the commit stores; rows are numbered in emission order -- and what each extension takes from it.
static void bank_plan_rows(kg_rxbank *b, int i, int nblk)
{
    bank_plan &p = b->plan;
    const int k = p.act[i];
    const bank_rx &r = b->rcv[k];
    const bool sam_family = p.mode[i] >= KG_POST_SAM && p.mode[i] <= KG_POST_QAM;
    kg_spec::emit_t m = r.spec_mirror;
    p.cmds[i] = kg_post_mode_cmds_(b->post, k);
    if (p.cmds[i] != r.spec_cmds) kg_spec::emit_clear(m);
    p.pb_n[i] = 0; p.pb_base[i] = 0;
    for (int blk = 0; blk < nblk; blk++) {
        const kg_spec::rows_t rows = kg_spec::emit_block(m, r.spec_on != 0, sam_family, p.sam_null[i] != 0);
        if (rows.passband) {                           // only ever the leading blocks: the mirror leaves PASSBAND once per step at most
            if (p.pb_n[i]++ == 0) p.pb_base[i] = p.nspec;
            p.spec_rx[p.nspec] = k; p.spec_inst[p.nspec] = KG_SPEC_PASSBAND; p.spec_blk[p.nspec] = blk; p.nspec++;
            p.any_pb = true;
        }
        p.null_row[(size_t) i * b->blocks_max + blk] = rows.chan_null ? p.nspec : -1;
        if (rows.chan_null) { p.spec_rx[p.nspec] = k; p.spec_inst[p.nspec] = KG_SPEC_CHAN_NULL; p.spec_blk[p.nspec] = blk; p.nspec++; }
    }
    p.mirror[i] = m;
    bank_fx_plan(b, i, nblk);
    bank_iq_plan(b, i, nblk);
    bank_lo_plan(b, i, nblk);
    bank_fa_plan(b, i, nblk);
    bank_cw_plan(b, i, nblk);
    bank_ws_plan(b, i, nblk);
    bank_f8_plan(b, i, nblk);
}

// The active list and, per entry, the counts its audio DDC and its CFastFIR will hand back (kg_rxddc_outputs is kg_rxddc_push_dev's
// own arithmetic, a CFastFIR call leaves (FirPos() + n) / 512 blocks), its mode, its blanker, its rows.  A receiver whose query refuses
// (no frequency set) is planned with nothing: the entry point says why.
static void bank_plan_audio(kg_rxbank *b)
{
    bank_plan &p = b->plan;
    for (std::vector<int32_t> *v : {&p.act, &p.nb_list, &p.nb_cnt}) v->clear();
    p.nrec_max = p.nfir_max = p.nspec = 0;
    p.any_pb = false;
    bank_fx_plan_clear(b);
    bank_iq_plan_clear(b);
    bank_lo_plan_clear(b);
    bank_fa_plan_clear(b);
    bank_cw_plan_clear(b);
    bank_ws_plan_clear(b);
    bank_f8_plan_clear(b);
    for (int k = 0; k < b->nrx; k++) {
        const bank_rx &r = b->rcv[k];
        p.enabled[k] = r.active ? 1 : 0;
        if (!r.active) continue;
        const int i = (int) p.act.size();
        p.act.push_back(k);
        const long outputs = kg_rxddc_outputs(b->rx, k, b->n);
        const int nrec = outputs > 0 ? (int) outputs : 0;
        const int nblk = (kg_fir_pos(b->fir, k) + nrec) / KG_FIR_OUT;
        p.nrec[i] = nrec; p.nfir[i] = nblk * KG_FIR_OUT;
        if (p.nrec[i] > p.nrec_max) p.nrec_max = p.nrec[i];
        if (p.nfir[i] > p.nfir_max) p.nfir_max = p.nfir[i];
        // the pre-filter blanker (rx_sound.cpp:593-598)
        if (r.nbc.snd_en[KG_NB_BLANKER] && r.nbc.algo == KG_NB_STD) { p.nb_list.push_back(k); p.nb_cnt.push_back(nrec); }
        p.mode[i] = kg_post_get_mode(b->post, k);
        p.sam_null[i] = p.mode[i] == KG_POST_SAM && (kg_post_sam_mparam_(b->post, k) & 3);
        bank_plan_rows(b, i, nblk);
    }
}

// One sound packet per 512 samples (rx_sound.cpp:601-1170): per sound block of the step the receivers that completed it, those of
// them whose nulled pair goes through m_chan_null_FIR (rx_sound.cpp:804, rows on or not), and who goes to which coder -- the real
// modes' blocks through the ADPCM coder, the stereo modes' (IS_STEREO: IQ, SAS, QAM) as (s2_t) pairs (rx_sound.cpp:1042-1140).
static void bank_plan_blocks(kg_rxbank *b)
{
    bank_plan &p = b->plan;
    const int NA = (int) p.act.size();
    for (std::vector<int32_t> *v : {&p.blk_chan, &p.blk_at, &p.blk_null_n, &p.blk_null_base}) v->clear();
    auto put = [&p](int k, int n, int base) { p.blk_chan.push_back(k); p.blk_null_n.push_back(n); p.blk_null_base.push_back(base); };
    for (int blk = 0; blk < p.nfir_max / KG_FIR_OUT; blk++)
        for (int j = 0; j < BL_N; j++) {
            p.blk_at.push_back((int32_t) p.blk_chan.size());
            for (int i = 0; i < NA; i++) {
                if (p.nfir[i] < (blk + 1) * KG_FIR_OUT) continue;
                const int k = p.act[i], m = p.mode[i], row = p.null_row[(size_t) i * b->blocks_max + blk];
                const bool stereo = bank_stereo(m), le = b->rcv[k].little_endian != 0;
                if (j == BL_POST || (j == BL_REAL && !stereo) || (j == BL_IQ_BE && stereo && !le) || (j == BL_IQ_LE && stereo && le)) put(k, 0, 0);
                if (j == BL_NULL && p.sam_null[i]) put(k, row >= 0 ? 1 : 0, row >= 0 ? row : 0);
            }
        }
    p.blk_at.push_back((int32_t) p.blk_chan.size());
}

// The waterfall chain: where each entry's DDC writes, which rings wrap first, which receivers have a frame and where it lies.
static void bank_plan_wf(kg_rxbank *b)
{
    bank_plan &p = b->plan;
    p.moves.clear();
    p.nframes = 0; p.wf_unset = -1;
    for (int i = 0; i < (int) p.act.size(); i++) {
        const int k = p.act[i];
        const bank_rx &r = b->rcv[k];
        long w = r.ring_w, total = r.ring_total;
        bool frame = true;
        p.out_off[i] = 0; p.max_out[i] = KG_WF_NFFT;
        uint64_t off = (uint64_t) k * b->wf_stride;
        if (!r.wf_set) {
            if (p.wf_unset < 0) p.wf_unset = k;
            frame = false;
        } else if (r.overlapped) {
            const long m = (long) (b->n / (size_t) r.decim);
            if (w + m > BANK_RING_PAIRS) {
                const long keep = KG_WF_NFFT - m;
                if (keep > 0) p.moves.push_back(bank_move{k, (int) (w - keep), 0, (int) keep});
                w = keep;
            }
            p.out_off[i] = w; p.max_out[i] = 0;
            w += m; total += m;
            frame = total >= KG_WF_NFFT;                                 // (before that: the reference sleeps, "fill pipe", :978)
            off += (uint64_t) (w - KG_WF_NFFT);
        }
        p.ring_w[i] = w; p.ring_total[i] = total;
        if (!frame) continue;
        p.chan_of[p.nframes] = k; p.frame_off[p.nframes] = off;
        p.pkt_step[p.nframes] = r.pkt;
        p.pkt_step[p.nframes].seq = r.snd_seq;                           // out->seq = wf->snd_seq, rx_waterfall.cpp:1635
        p.nframes++;
    }
}

static void bank_plan_step(kg_rxbank *b)
{
    bank_plan_audio(b);
    bank_plan_blocks(b);
    bank_plan_wf(b);
}

// ---- enqueue: the entry points in the order their tables sit in the slot.  Reads the plan; decides and commits nothing.

// An edge of the stream graph, and the one place that tells the two passes apart: the PLAN pass enqueues none.  `from` records ev
// (null: an earlier step did, if *pending), `to` waits for it (null: the next step's reader will, so *pending is set).
static int bank_edge(bool real, hipEvent_t ev, hipStream_t from, hipStream_t to, bool *pending = nullptr)
{
    if (!real) return KG_OK;
    if (from) KG_HIP(hipEventRecord(ev, from));
    if (to && (from || *pending)) KG_HIP(hipStreamWaitEvent(to, ev, 0));
    if (pending) *pending = from != nullptr;
    return KG_OK;
}

static bool bank_real(const kg_rxbank *b) { return b->arena.mode != KG_ARENA_PLAN; }

// what an entry point handed back against what the plan counted
static int bank_counts_agree(const bank_plan &p, const std::vector<int32_t> &plan, const std::vector<int32_t> &got, const char *what, const char *who)
{
    for (size_t i = 0; i < p.act.size(); i++)
        KG_REQUIRE(got[i] == plan[i], KG_ERR_STATE, "kg_rxbank_step: receiver %d: %d %s planned, %s hands back %d", p.act[i], plan[i], what, who,
                   got[i]);
    return KG_OK;
}

// the step's ring moves, staged and launched the way an entry point does it
static int bank_moves_dev(kg_rxbank *b)
{
    const bank_plan &p = b->plan;
    void *d_mv = nullptr;
    KG_TRY(kg_ctx_stage(b->c_main, p.moves.data(), sizeof(bank_move) * p.moves.size(), &d_mv));
    KG_PLAN_ONLY(b->c_main);
    hipLaunchKernelGGL(rxbank_move_kernel, dim3((unsigned) p.moves.size()), dim3(256), 0, b->s_main, b->d_wfiq, (long) b->wf_stride,
                       (const bank_move *) d_mv);
    KG_HIP(hipGetLastError());
    return KG_OK;
}

// audio chain (side stream): rx.v -> rx_iq_t -> snd_service() unpack -> the pre-filter blanker -> CFastFIR
static int bank_audio_front(kg_rxbank *b, const void *d_adc)
{
    bank_plan &p = b->plan;
    const int NA = (int) p.act.size(), NR = b->nrx;
    if (NA == 0) return KG_OK;
    const bool real = bank_real(b);
    const int32_t *act = p.act.data();
    bank_tick tk;
    KG_TRY(kg_rxddc_push_dev(b->rx, d_adc, b->n, act, NA, b->d_raw, b->nrec_max, p.got_nrec.data()));
    KG_TRY(bank_counts_agree(p, p.nrec, p.got_nrec, "records", "kg_rxddc_push_dev"));
    tk.lap(b, PF_RXDDC, real);
    // (rows are unpacked up to the largest count of the step; a receiver's CFastFIR takes its own count of them)
    if (p.nrec_max > 0)
        KG_TRY(kg_dpump_unpack_rows_dev(b->c_side, b->d_raw, b->nrec_max, p.nrec_max, NR, p.enabled.data(), b->rescale, b->dc_i, b->dc_q,
                                        b->spectral_inversion, b->d_xin, b->nrec_max));
    if (!p.nb_list.empty())                                // in place on the unpacked rows, before CFastFIR
        KG_TRY(kg_nb_process_dev(b->nb, p.nb_list.data(), (int) p.nb_list.size(), b->d_xin, b->nrec_max, p.nb_cnt.data(), b->d_xin, b->nrec_max));
    tk.lap(b, PF_UNPACK, real);
    KG_TRY(bank_edge(real, b->ev_tail, nullptr, b->s_side, &b->tail_pending));     // the coders of the step before have read fir_out
    tk.lap(b, PF_EVENTS, real);
    const kg_fir_spec_req req = {b->d_spec, KG_SPEC_ROW, b->spec_max * KG_SPEC_ROW, p.pb_inst.data(), p.pb_n.data(), p.pb_base.data()};
    int rc;
    if (!b->fx.plan.list.empty())                          // the FFT extension's entries: the filter stores its spectra for them, by list entry
        rc = kg_fir_process_post_(b->fir, act, NA, b->d_xin, b->nrec_max, p.nrec.data(), b->d_firo, b->firo_stride, p.got_nfir.data(),
                                  p.any_pb ? &req : nullptr, b->fx.d_post, b->fx.stride);
    else if (p.any_pb)
        rc = kg_fir_process_rows_(b->fir, act, NA, b->d_xin, b->nrec_max, p.nrec.data(), b->d_firo, b->firo_stride, p.got_nfir.data(), &req);
    else
        rc = kg_fir_process_each_dev(b->fir, act, NA, b->d_xin, b->nrec_max, p.nrec.data(), b->d_firo, b->firo_stride, p.got_nfir.data());
    if (rc) return rc;
    KG_TRY(bank_counts_agree(p, p.nfir, p.got_nfir, "CFastFIR outputs", "kg_fir"));
    tk.lap(b, PF_FIR, real);
    return KG_OK;
}

// the tail stream, per sound block: S-meter, CAgc, detector; the channel-null filter; the coders.  Then the extensions' launches, ahead of ev_tail.
static int bank_audio_tail(kg_rxbank *b)
{
    bank_plan &p = b->plan;
    if (p.nfir_max == 0) return KG_OK;
    const bool real = bank_real(b), fx = !b->fx.plan.list.empty();
    const size_t NR = (size_t) b->nrx;
    bank_tick tk;
    KG_TRY(bank_edge(real, b->ev_fir, b->s_side, b->s_tail));
    tk.lap(b, PF_EVENTS, real);
    for (int blk = 0; blk < p.nfir_max / KG_FIR_OUT; blk++) {
        const size_t o = (size_t) blk * KG_FIR_OUT;
        const int32_t *chan = p.blk_chan.data();
        KG_TRY(kg_post_process_dev(b->post, chan + p.at(blk, BL_POST), p.count(blk, BL_POST), b->d_firo + o, b->firo_stride, KG_FIR_OUT, b->d_s16 + o,
                                   nullptr, b->d_agc + o, b->firo_stride));
        if (const int NN = p.count(blk, BL_NULL)) {        // without an output buffer; with the extension on, block blk of the channel-null spectra
            const int at = p.at(blk, BL_NULL);
            const kg_fir_spec_req req = {b->d_spec, KG_SPEC_ROW, b->spec_max * KG_SPEC_ROW, p.null_inst.data(), p.blk_null_n.data() + at,
                                         p.blk_null_base.data() + at};
            if (fx)
                KG_TRY(kg_fir_process_post_(b->nullfir, chan + at, NN, b->d_agc + o, b->firo_stride, p.null_each.data(), nullptr, 0, nullptr, &req,
                                            b->fx.d_post + (NR * b->blocks_max + (size_t) blk * NR) * KG_FFTEXT_ROW, KG_FFTEXT_ROW));
            else
                KG_TRY(kg_fir_process_rows_(b->nullfir, chan + at, NN, b->d_agc + o, b->firo_stride, p.null_each.data(), nullptr, 0, nullptr, &req));
        }
        tk.lap(b, PF_POST, real);
        if (const int NL = p.count(blk, BL_REAL))
            KG_TRY(kg_adpcm_encode_dev(b->adpcm, chan + p.at(blk, BL_REAL), NL, b->d_s16 + o, b->firo_stride, KG_FIR_OUT, b->d_pay + o / 2,
                                       b->firo_stride / 2));
        for (int le = 0; le < 2; le++)                     // SAS / QAM leave their (L, R) pair in the agc buffer
            if (const int NL = p.count(blk, BL_IQ_BE + le))
                KG_TRY(kg_snd_iq_payload_dev(b->c_tail, chan + p.at(blk, BL_IQ_BE + le), NL, b->d_agc + o, b->firo_stride, KG_FIR_OUT, le,
                                             b->d_iqpay + 4 * o, 4 * b->firo_stride));
        tk.lap(b, PF_ADPCM, real);
    }
    KG_TRY(bank_fx_enqueue(b));
    KG_TRY(bank_iq_enqueue(b));
    KG_TRY(bank_lo_enqueue(b));
    KG_TRY(bank_fa_enqueue(b));
    KG_TRY(bank_cw_enqueue(b));
    KG_TRY(bank_ws_enqueue(b));
    KG_TRY(bank_f8_enqueue(b));
    KG_TRY(bank_edge(real, b->ev_tail, b->s_tail, nullptr, &b->tail_pending));
    tk.lap(b, PF_EVENTS, real);
    return KG_OK;
}

// waterfall chain (main stream): ring moves, DDC, frames; the packets on the tail stream
static int bank_wf_chain(kg_rxbank *b, const void *d_adc)
{
    bank_plan &p = b->plan;
    const int NA = (int) p.act.size();
    const bool real = bank_real(b);
    bank_tick tk;
    KG_REQUIRE(p.wf_unset < 0, KG_ERR_STATE, "kg_rxbank_step: kg_rxbank_set_wf was not called for receiver %d (since it joined)", p.wf_unset);
    if (!p.moves.empty()) KG_TRY(bank_moves_dev(b));
    if (NA > 0)
        KG_TRY(kg_ddc_wf_step_dev(b->ddc, d_adc, b->n, p.act.data(), NA, b->d_wfiq, b->wf_stride, p.out_off.data(), p.max_out.data(), p.h_nw.data()));
    tk.lap(b, PF_DDC, real);
    KG_TRY(bank_edge(real, b->ev_pk, nullptr, b->s_main, &b->pk_pending));         // the packets of the step before have read the rows
    tk.lap(b, PF_EVENTS, real);
    if (p.nframes == 0) return KG_OK;
    KG_TRY(kg_wf_frames_at_dev(b->wf, p.nframes, p.chan_of.data(), p.frame_off.data(), (uint64_t) b->nrx * b->wf_stride, b->d_wfiq, b->d_rows));
    tk.lap(b, PF_FRAMES, real);
    KG_TRY(bank_edge(real, b->ev_frames, b->s_main, b->s_tail));
    tk.lap(b, PF_EVENTS, real);
    KG_TRY(kg_wf_packets_dev(b->c_tail, b->d_rows, KG_WF_WIDTH, p.nframes, p.pkt_step.data(), b->d_pkts, BANK_PKT_STRIDE, p.pkt_bytes.data()));
    tk.lap(b, PF_PKT, real);
    KG_TRY(bank_edge(real, b->ev_pk, b->s_tail, nullptr, &b->pk_pending));
    tk.lap(b, PF_EVENTS, real);
    return KG_OK;
}

static int bank_pass(kg_rxbank *b, const void *d_adc)
{
    KG_TRY(bank_audio_front(b, d_adc));
    KG_TRY(bank_audio_tail(b));
    return bank_wf_chain(b, d_adc);
}

// ---- commit: the step has been enqueued; the plan's next values and maps become the bank's
static void bank_commit(kg_rxbank *b)
{
    bank_plan &p = b->plan;
    const int NA = (int) p.act.size();
    kg_rxbank_step_info &s = b->last;
    const int first = NA > 0 ? p.act[0] : 0;               // the step's scalar audio fields: the lowest-numbered active receiver's
    s.step = b->step; s.nframes = p.nframes; s.nrec = NA > 0 ? p.nrec[0] : 0; s.nfir = NA > 0 ? p.nfir[0] : 0;
    s.fir_pos = kg_fir_pos(b->fir, first);
    s.snd_seq = b->rcv[first].snd_seq; s.table_bytes = (int32_t) b->arena.used; s.nmoves = (int32_t) p.moves.size();
    for (bank_rx &r : b->rcv) { r.last_nrec = 0; r.last_nfir = 0; }
    for (int i = 0; i < NA; i++) {
        bank_rx &r = b->rcv[p.act[i]];
        r.ring_w = p.ring_w[i]; r.ring_total = p.ring_total[i];
        r.spec_mirror = p.mirror[i]; r.spec_cmds = p.cmds[i];
        r.last_nrec = p.nrec[i]; r.last_nfir = p.nfir[i];
        r.snd_seq += (uint32_t) (p.nfir[i] / KG_FIR_OUT);
    }
    b->spec_n = p.nspec;
    b->spec_rx.swap(p.spec_rx); b->spec_inst.swap(p.spec_inst); b->spec_blk.swap(p.spec_blk);
    bank_fx_commit(b);
    bank_iq_commit(b);
    bank_lo_commit(b);
    bank_fa_commit(b);
    bank_cw_commit(b);
    bank_ws_commit(b);
    bank_f8_commit(b);
    b->frame_rx.swap(p.chan_of); b->frame_off.swap(p.frame_off); b->pkt_bytes.swap(p.pkt_bytes);
}

// `SET zoom=` with a new zoom (rx_waterfall.cpp:460): the waterfall blanker is set up again before the next frame
static void bank_nb_zoom_change(kg_rxbank *b, int rx)
{
    bank_nb_cmd &c = b->rcv[rx].nbc;
    if (c.wf_en[KG_NB_BLANKER] && c.wf_en[KG_NB_WF]) c.wf_change[KG_NB_BLANKER] = 1;
}

// SetupBlanker's refusals for a parameter vector at `rate`, without touching any blanker
static int bank_nb_check(const float *prm, float rate, const char *who)
{
    kg_nbk::st t{};
    const int r = kg_nbk::setup(t, true, rate, prm);
    KG_REQUIRE(r == kg_nbk::SETUP_OK, KG_ERR_INVALID, "%s: gate %g us / threshold %g at %g Hz is refused (kg_nb_setup)", who,
               (double) prm[KG_NB_GATE], (double) prm[KG_NB_THRESHOLD], (double) rate);
    return KG_OK;
}

// `SET nb algo=` (rx_sound_cmd.cpp:454-462): the algo, both sides' enables cleared, no blanker state touched.  With the audio enable
// gone the Wild stage is off whatever the new algo.
static int bank_nb_algo(kg_rxbank *b, int rx, int algo)
{
    int rc = kg_post_set_nbw(b->post, rx, 0);
    if (rc) return rc;
    bank_nb_cmd &c = b->rcv[rx].nbc;
    c.algo = algo;
    memset(c.snd_en, 0, sizeof c.snd_en);
    memset(c.wf_en, 0, sizeof c.wf_en);
    return KG_OK;
}

extern "C" {

int kg_rxbank_set_nb_algo(kg_rxbank *b, int rx, int algo)
{
    KG_TRY(bank_rx_check(b, rx, "kg_rxbank_set_nb_algo"));
    KG_REQUIRE(algo == KG_NB_OFF || algo == KG_NB_STD, KG_ERR_INVALID, "kg_rxbank_set_nb_algo: algo %d (%s)", algo,
               algo == KG_NB_WILD ? "NB_WILD is selected by kg_rxbank_nbw_select" : "not an nb_algo_e");
    return bank_nb_algo(b, rx, algo);
}

int kg_rxbank_nbw_select(kg_rxbank *b, int rx)
{
    KG_TRY(bank_rx_check(b, rx, "kg_rxbank_nbw_select"));
    return bank_nb_algo(b, rx, KG_NB_WILD);
}

int kg_rxbank_set_nb_enable(kg_rxbank *b, int rx, int type, int en)
{
    int rc = bank_rx_check(b, rx, "kg_rxbank_set_nb_enable");
    if (rc) return rc;
    KG_REQUIRE(type >= 0 && type < 4, KG_ERR_INVALID, "kg_rxbank_set_nb_enable: type %d (0..3)", type);
    KG_REQUIRE(!(type == KG_NB_CLICK && en), KG_ERR_INVALID, "kg_rxbank_set_nb_enable: NB_CLICK test pulses are not implemented");
    bank_nb_cmd &c = b->rcv[rx].nbc;
    KG_REQUIRE(!(type == KG_NB_BLANKER && en && c.algo == KG_NB_STD && !kg_nb_was_setup(b->nb, rx)), KG_ERR_STATE,
               "kg_rxbank_set_nb_enable: receiver %d's audio blanker was never set up (send its parameters first)", rx);
    if (type == KG_NB_BLANKER && c.algo == KG_NB_WILD && (rc = kg_post_set_nbw(b->post, rx, en))) return rc;   // rx_sound.cpp:924-929
    c.snd_en[type] = en;                                                         // rx_sound_cmd.cpp:477-483
    c.wf_en[type] = en;
    return KG_OK;
}

int kg_rxbank_set_nb_param(kg_rxbank *b, int rx, int type, int param, float pval, float frate)
{
    int rc = bank_rx_check(b, rx, "kg_rxbank_set_nb_param");
    if (rc) return rc;
    KG_REQUIRE(type >= 0 && type < 4 && param >= 0 && param < 8, KG_ERR_INVALID, "kg_rxbank_set_nb_param: type %d param %d", type, param);
    bank_nb_cmd &c = b->rcv[rx].nbc;
    float snd[8], wfp[8];
    memcpy(snd, c.snd_param[type], sizeof snd);
    memcpy(wfp, c.wf_param[type], sizeof wfp);
    snd[param] = pval;
    wfp[param] = pval;
    const bool to_wf = c.algo == KG_NB_STD || type == KG_NB_CLICK;               // rx_sound_cmd.cpp:491-494
    const bool setup = type == KG_NB_BLANKER && c.algo == KG_NB_STD;              // :496-500
    if (setup && (rc = bank_nb_check(snd, frate, "kg_rxbank_set_nb_param"))) return rc;
    if (to_wf && type == KG_NB_BLANKER && (rc = bank_nb_check(wfp, (float) KG_WF_NFFT, "kg_rxbank_set_nb_param"))) return rc;
    if (setup && (rc = kg_nb_setup(b->nb, rx, frate, snd))) return rc;           // SetupBlanker("SND", frate, ...)
    if (type == KG_NB_BLANKER && c.algo == KG_NB_WILD && (rc = kg_post_nbw_init(b->post, rx, snd))) return rc;   // :498: nb_Wild_init
    c.snd_param[type][param] = pval;
    if (to_wf) {
        c.wf_param[type][param] = pval;
        c.wf_change[type] = 1;
    }
    return KG_OK;
}

int kg_rxbank_set_nb_gate(kg_rxbank *b, int rx, int nb, int th, float frate)
{
    int rc = bank_rx_check(b, rx, "kg_rxbank_set_nb_gate");
    if (rc) return rc;
    bank_nb_cmd &c = b->rcv[rx].nbc;
    float snd[8];
    memcpy(snd, c.snd_param[KG_NB_BLANKER], sizeof snd);
    snd[KG_NB_GATE] = nb;                                                        // rx_sound_cmd.cpp:660-672
    snd[KG_NB_THRESHOLD] = th;
    if (nb && (rc = bank_nb_check(snd, frate, "kg_rxbank_set_nb_gate"))) return rc;
    // under NB_WILD the command changes the enable and never calls nb_Wild_init: the stage keeps the vector of its last init
    if (c.algo == KG_NB_WILD && (rc = kg_post_set_nbw(b->post, rx, nb ? 1 : 0))) return rc;
    if (nb && (rc = kg_nb_setup(b->nb, rx, frate, snd))) return rc;
    memcpy(c.snd_param[KG_NB_BLANKER], snd, sizeof snd);
    c.snd_en[KG_NB_BLANKER] = nb ? 1 : 0;
    return KG_OK;
}

int kg_rxbank_nb_cmd_state(kg_rxbank *b, int rx, int32_t *ints, float *flts)
{
    KG_TRY(bank_rx_check(b, rx, "kg_rxbank_nb_cmd_state"));
    const bank_nb_cmd &c = b->rcv[rx].nbc;
    if (ints) {
        ints[0] = c.algo;
        for (int t = 0; t < 4; t++) { ints[1 + t] = c.snd_en[t]; ints[5 + t] = c.wf_en[t]; ints[9 + t] = c.wf_change[t]; }
        ints[13] = c.wf_setup;
    }
    if (flts) { memcpy(flts, c.snd_param, sizeof c.snd_param); memcpy(flts + 32, c.wf_param, sizeof c.wf_param); }
    return KG_OK;
}

}  // extern "C"

// The four streams that carry kernels are created back to back, the upload's fifth.  Which hardware queue (and, behind
// it, which of the four dispatch pipes) a stream lands on is the HIP runtime's choice -- the least-shared queue of its pool
// at that moment -- and depends on every stream the process created before: measured on one bank, 0.98 ms per step or
// 1.25 ... 1.38 by what had run earlier in the process (tools/micro/stream_pairs.hip measures which pairs of
// streams run side by side).  Creating them together at least keeps them off one another's queues while the pool has
// free ones.
static int bank_streams(kg_rxbank *b)
{
    {
        std::lock_guard<std::mutex> lk(g_free_mutex);
        for (size_t i = 0; i < g_free_sets.size(); i++)
            if (g_free_sets[i].device == b->device) {
                const bank_stream_set st = g_free_sets[i];
                g_free_sets.erase(g_free_sets.begin() + (long) i);
                b->s_main = st.s[0]; b->s_side = st.s[1]; b->s_tail = st.s[2]; b->s_ddc_side = st.s[3]; b->s_up = st.s[4];
                return KG_OK;
            }
    }
    for (hipStream_t *st : {&b->s_main, &b->s_side, &b->s_tail, &b->s_ddc_side, &b->s_up}) KG_HIP(hipStreamCreateWithFlags(st, hipStreamNonBlocking));
    return KG_OK;
}

template <class T> static int bank_zalloc(kg_dbuf<T> &d, size_t count, const char *what)
{
    KG_TRY(d.alloc(count, what));
    KG_HIP(hipMemset(d, 0, sizeof(T) * count));
    return KG_OK;
}

// the contexts, the per-seam objects and the device buffers
static int bank_alloc(kg_rxbank *b)
{
    const int device = b->device, nrx = b->nrx;
    KG_TRY(kg_ctx_create_on_stream(device, b->s_main, &b->c_main));
    KG_TRY(kg_ctx_create_on_stream(device, b->s_side, &b->c_side));
    KG_TRY(kg_ctx_create_on_stream(device, b->s_tail, &b->c_tail));
    KG_TRY(kg_ddc_create(b->c_main, nrx, b->n, &b->ddc));
    KG_TRY(kg_ddc_use_side_stream(b->ddc, b->s_ddc_side));
    KG_TRY(kg_wf_create(b->c_main, nrx, &b->wf));
    KG_TRY(kg_rxddc_create_mode(b->c_side, nrx, b->n, b->mode, &b->rx));
    b->decim_rx = kg_rxddc_decim(b->rx);
    b->nrec_max = b->n / (size_t) b->decim_rx + 2;
    KG_TRY(kg_fir_create(b->c_side, nrx, (int) b->nrec_max, &b->fir));
    KG_TRY(kg_nb_create(b->c_side, nrx, (int) b->nrec_max, &b->nb));
    KG_TRY(kg_post_create(b->c_tail, nrx, &b->post));
    KG_TRY(kg_adpcm_create(b->c_tail, nrx, &b->adpcm));
    KG_TRY(kg_fir_create(b->c_tail, nrx, KG_FIR_OUT, &b->nullfir));
    b->wf_stride = BANK_RING_PAIRS;
    b->firo_stride = ((b->nrec_max + KG_FIR_OUT - 1) / KG_FIR_OUT + 1) * KG_FIR_OUT;
    KG_TRY(bank_zalloc(b->d_wfiq, b->wf_stride * nrx, "kg_rxbank_create: wfiq"));
    KG_TRY(bank_zalloc(b->d_rows, (size_t) KG_WF_WIDTH * nrx, "kg_rxbank_create: rows"));
    KG_TRY(bank_zalloc(b->d_pkts, (size_t) BANK_PKT_STRIDE * nrx, "kg_rxbank_create: pkts"));
    KG_TRY(b->d_raw.alloc(6 * b->nrec_max * nrx, "kg_rxbank_create: raw"));
    KG_TRY(b->d_xin.alloc(b->nrec_max * nrx, "kg_rxbank_create: xin"));
    KG_TRY(b->d_firo.alloc(b->firo_stride * nrx, "kg_rxbank_create: firo"));
    KG_TRY(bank_zalloc(b->d_s16, b->firo_stride * nrx, "kg_rxbank_create: s16"));
    KG_TRY(bank_zalloc(b->d_pay, b->firo_stride / 2 * nrx, "kg_rxbank_create: pay"));
    KG_TRY(bank_zalloc(b->d_agc, b->firo_stride * nrx, "kg_rxbank_create: agc"));
    KG_TRY(bank_zalloc(b->d_iqpay, 4 * b->firo_stride * nrx, "kg_rxbank_create: iqpay"));
    return KG_OK;
}

// the plan's arrays at the size of the largest step: per receiver, per (receiver, sound block), per row
static void bank_plan_init(bank_plan &p, size_t nrx, size_t blocks_max, size_t spec_max)
{
    for (std::vector<int32_t> *v : {&p.nrec, &p.nfir, &p.mode, &p.pb_n, &p.pb_base, &p.chan_of, &p.got_nrec, &p.got_nfir, &p.pkt_bytes}) v->assign(nrx, 0);
    for (std::vector<int32_t> *v : {&p.spec_rx, &p.spec_inst, &p.spec_blk}) v->assign(spec_max, 0);
    for (std::vector<int32_t> *v : {&p.act, &p.nb_list, &p.nb_cnt}) v->reserve(nrx);
    for (std::vector<int32_t> *v : {&p.blk_chan, &p.blk_null_n, &p.blk_null_base}) v->reserve(3 * nrx * blocks_max);
    p.blk_at.reserve(BL_N * blocks_max + 1);
    p.pb_inst.assign(nrx, KG_SPEC_PASSBAND); p.null_inst.assign(nrx, KG_SPEC_CHAN_NULL); p.null_each.assign(nrx, KG_FIR_OUT);
    p.null_row.assign(blocks_max * nrx, -1);
    p.enabled.assign(nrx, 1); p.sam_null.assign(nrx, 0);
    p.moves.reserve(nrx); p.out_off.assign(nrx, 0); p.max_out.assign(nrx, 0); p.h_nw.assign(nrx, 0);
    p.frame_off.assign(nrx, 0); p.pkt_step.resize(nrx);
    p.ring_w.assign(nrx, 0); p.ring_total.assign(nrx, 0); p.mirror.assign(nrx, kg_spec::emit_t{KG_SPEC_PASSBAND}); p.cmds.assign(nrx, 0);
    p.nrec_max = p.nfir_max = p.nspec = p.nframes = 0; p.wf_unset = -1; p.any_pb = false;
}

static int bank_init(kg_rxbank *b)
{
    const int nrx = b->nrx;
    KG_TRY(bank_streams(b));
    KG_TRY(bank_alloc(b));
    {   // what a step's tables can take: <= 12 of them + a channel list for S-meter / AGC / detector and one for the coder per sound
        // block (a receiver can complete nrec_max / 512 + 1 blocks in a step) -- checked HERE, not found out by every later step
        // (+ one for the channel-null filter per sound block)
        const size_t blocks_max = b->blocks_max = b->nrec_max / KG_FIR_OUT + 1;
        if (16 + 5 * blocks_max > KG_ARENA_MAX_ENTRIES) {
            kg_set_error("kg_rxbank_create: %zu ADC samples per step are up to %zu sound blocks per receiver and step; the step table holds %d "
                         "(a step of at most %zu samples)", b->n, blocks_max, (KG_ARENA_MAX_ENTRIES - 16) / 5,
                         (size_t) ((KG_ARENA_MAX_ENTRIES - 16) / 5 - 1) * KG_FIR_OUT * (size_t) b->decim_rx);
            return KG_ERR_INVALID;
        }
        // (+ 64 per receiver: the blankers' tables; the audio spectrum: 12 bytes per receiver in CFastFIR's table, and per sound block
        // the channel-null filter's table of 8 ints per receiver and its alignment; + 64 per table -- up to 12 and 4 per sound
        // block -- for the 64-byte alignment arena_stage gives every entry)
        // (+ the FFT extension's table: 2 groups of 32 bytes and 2 ops of 16 per sound block, per receiver)
        // (+ the IQ display's table: a group of 112 bytes per receiver, an op of 32 per sound block, and its alignment)
        b->slot_bytes = (8192 + 64 + 64 * blocks_max + 64 * (13 + 4 * blocks_max) + (size_t) (448 + 16 + 64 + 112 + (12 + 32 + 32 + 32) * blocks_max) * nrx + 63) &
                        ~(size_t) 63;
        b->spec_max = 2 * blocks_max * (size_t) nrx;                         // a passband and a channel-null row per sound block
    }
    KG_TRY(b->h_slots.alloc(b->slot_bytes * BANK_SLOTS, "kg_rxbank_create: slots"));
    KG_TRY(b->d_slots.alloc(b->slot_bytes * BANK_SLOTS, "kg_rxbank_create: slots"));
    for (int i = 0; i < BANK_SLOTS; i++) {
        // hipEventBlockingSync: a host that has run BANK_SLOTS steps ahead SLEEPS in kg_rxbank_step's slot wait instead of spinning
        // (the reference's server is one cooperative thread: it asks kg_rxbank_ready first and yields instead)
        for (int j = 0; j < 3; j++) KG_HIP(hipEventCreateWithFlags(&b->ev_end[i][j], hipEventDisableTiming | hipEventBlockingSync));
        b->ev_end_rec[i] = false;
    }
    for (hipEvent_t *e : {&b->ev_tab, &b->ev_fir, &b->ev_tail, &b->ev_frames, &b->ev_pk})
        KG_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    // rescale = MPOW(2, -RXOUT_SCALE + CUTESDR_SCALE) * MPOW(10, CICF_GAIN_dB / 20), rx/data_pump.cpp:73-74 (kg_rxbank_set_unpack overrides)
    b->rescale = powf(2.f, -23 + 15) * powf(10.f, 4.5f / 20.f); b->dc_i = b->dc_q = 0.f; b->spectral_inversion = 0;
    b->tail_pending = b->pk_pending = false; b->step = 0;
    b->c_main->rows_by_chan = b->c_side->rows_by_chan = b->c_tail->rows_by_chan = 1;      // buffers hold one row per RECEIVER
    KG_TRY(bank_zalloc(b->d_spec, b->spec_max * KG_SPEC_ROW, "kg_rxbank_create: spec"));
    b->rcv.assign(nrx, bank_rx{});
    bank_plan_init(b->plan, (size_t) nrx, b->blocks_max, b->spec_max);
    b->spec_n = 0;
    bank_fx_sizes(b);
    bank_iq_sizes(b);
    bank_lo_sizes(b);
    bank_fa_sizes(b);
    bank_cw_sizes(b);
    bank_ws_sizes(b);
    bank_f8_sizes(b);
    for (std::vector<int32_t> *v : {&b->spec_rx, &b->spec_inst, &b->spec_blk}) v->assign(b->spec_max, 0);
    b->frame_rx.assign(nrx, -1); b->pkt_bytes.assign(nrx, 0); b->frame_off.assign(nrx, 0);
    memset(&b->arena, 0, sizeof b->arena);
    memset(&b->last, 0, sizeof b->last);
    KG_HIP(hipDeviceSynchronize());
    return KG_OK;
}

extern "C" {

void kg_rxbank_destroy(kg_rxbank *b)
{
    if (!b) return;
    (void) hipSetDevice(b->device);
    for (hipStream_t s : {b->s_main, b->s_side, b->s_tail, b->s_ddc_side, b->s_up}) if (s) (void) hipStreamSynchronize(s);
    if (b->c_main && b->c_side && b->c_tail) bank_set_arena(b, KG_ARENA_OFF);
    kg_fftext_destroy(b->fx.obj);
    kg_iqd_destroy(b->iq.obj);
    kg_lorc_destroy(b->lo.obj);
    kg_fax_destroy(b->fa.obj);
    kg_cw_destroy(b->cw.obj);
    kg_wspr_destroy(b->ws.obj);
    kg_ft8_destroy(b->f8.obj);
    kg_adpcm_destroy(b->adpcm); kg_post_destroy(b->post); kg_fir_destroy(b->nullfir); kg_fir_destroy(b->fir); kg_rxddc_destroy(b->rx); kg_nb_destroy(b->nb);
    kg_wf_destroy(b->wf); kg_ddc_destroy(b->ddc);
    kg_ctx_destroy(b->c_tail); kg_ctx_destroy(b->c_side); kg_ctx_destroy(b->c_main);
    for (int i = 0; i < BANK_SLOTS; i++) for (int j = 0; j < 3; j++) if (b->ev_end[i][j]) (void) hipEventDestroy(b->ev_end[i][j]);
    for (hipEvent_t e : {b->ev_tab, b->ev_fir, b->ev_tail, b->ev_frames, b->ev_pk}) if (e) (void) hipEventDestroy(e);
    if (b->s_main && b->s_side && b->s_tail && b->s_ddc_side && b->s_up) {          // a complete set: kept for the next bank
        std::lock_guard<std::mutex> lk(g_free_mutex);
        g_free_sets.push_back(bank_stream_set{b->device, {b->s_main, b->s_side, b->s_tail, b->s_ddc_side, b->s_up}});
    } else {
        for (hipStream_t s : {b->s_main, b->s_side, b->s_tail, b->s_ddc_side, b->s_up}) if (s) (void) hipStreamDestroy(s);
    }
    delete b;
}

int kg_rxbank_create(int device, int nrx, size_t adc_samples_per_step, int rx_mode, kg_rxbank **out)
{
    KG_REQUIRE(out != nullptr, KG_ERR_INVALID, "kg_rxbank_create: out is null");
    *out = nullptr;
    KG_REQUIRE(nrx >= 1 && nrx <= 4096, KG_ERR_INVALID, "kg_rxbank_create: nrx %d (1..4096)", nrx);
    KG_REQUIRE(adc_samples_per_step >= 8192 && adc_samples_per_step <= ((size_t) 1 << 27), KG_ERR_INVALID,
               "kg_rxbank_create: %zu ADC samples per step (8192 .. 2^27)", adc_samples_per_step);
    {   // (what says "no gfx950 device": there is no CPU fallback)
        int ndev = 0;
        const hipError_t e = hipGetDeviceCount(&ndev);
        KG_REQUIRE(e == hipSuccess && ndev > 0, KG_ERR_NO_DEVICE, "kg_rxbank_create: no HIP device (%s); libkiwigpu has no CPU fallback",
                   e == hipSuccess ? "device count 0" : hipGetErrorString(e));
        KG_REQUIRE(device >= 0 && device < ndev, KG_ERR_INVALID, "kg_rxbank_create: device %d out of range (0..%d)", device, ndev - 1);
    }
    KG_HIP(hipSetDevice(device));
    {
        hipDeviceProp_t prop;
        KG_HIP(hipGetDeviceProperties(&prop, device));
        KG_REQUIRE(strncmp(prop.gcnArchName, "gfx950", 6) == 0, KG_ERR_NO_DEVICE,
                   "kg_rxbank_create: device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
    }
    kg_rxbank *b = new (std::nothrow) kg_rxbank();
    KG_REQUIRE(b != nullptr, KG_ERR_NOMEM, "kg_rxbank_create: alloc");
    b->device = device; b->nrx = nrx; b->mode = rx_mode; b->n = adc_samples_per_step;
    const int rc = bank_init(b);
    if (rc) { kg_rxbank_destroy(b); return rc; }
    *out = b;
    return KG_OK;
}

kg_ddc *kg_rxbank_ddc(kg_rxbank *b) { return b ? b->ddc : nullptr; }
kg_wf *kg_rxbank_wf(kg_rxbank *b) { return b ? b->wf : nullptr; }
kg_rxddc *kg_rxbank_rxddc(kg_rxbank *b) { return b ? b->rx : nullptr; }
kg_fir *kg_rxbank_fir(kg_rxbank *b) { return b ? b->fir : nullptr; }
kg_post *kg_rxbank_post(kg_rxbank *b) { return b ? b->post : nullptr; }
kg_adpcm *kg_rxbank_adpcm(kg_rxbank *b) { return b ? b->adpcm : nullptr; }
kg_ctx *kg_rxbank_ctx(kg_rxbank *b) { return b ? b->c_main : nullptr; }
kg_nb *kg_rxbank_nb(kg_rxbank *b) { return b ? b->nb : nullptr; }
kg_fir *kg_rxbank_null_fir(kg_rxbank *b) { return b ? b->nullfir : nullptr; }

// `SET spc_=%d` (rx_sound_cmd.cpp:332-339)
int kg_rxbank_set_spec(kg_rxbank *b, int rx, int n)
{
    KG_TRY(bank_rx_check(b, rx, "kg_rxbank_set_spec"));
    b->rcv[rx].spec_on = kg_spec::cmd_on(n) ? 1 : 0;
    return KG_OK;
}

int kg_rxbank_spec_max(kg_rxbank *b)
{
    KG_REQUIRE(b != nullptr, KG_ERR_INVALID, "kg_rxbank_spec_max: null argument");
    return (int) b->spec_max;
}

int kg_rxbank_spec_map(kg_rxbank *b, int32_t *rx_of_row, int32_t *inst_of_row, int32_t *blk_of_row)
{
    KG_REQUIRE(b != nullptr, KG_ERR_INVALID, "kg_rxbank_spec_map: null argument");
    for (int r = 0; r < b->spec_n; r++) {
        if (rx_of_row) rx_of_row[r] = b->spec_rx[r];
        if (inst_of_row) inst_of_row[r] = b->spec_inst[r];
        if (blk_of_row) blk_of_row[r] = b->spec_blk[r];
    }
    return b->spec_n;
}

int kg_rxbank_spec_rows(kg_rxbank *b, void **d_rows, size_t *row_stride)
{
    KG_REQUIRE(b && d_rows && row_stride, KG_ERR_INVALID, "kg_rxbank_spec_rows: null argument");
    *d_rows = b->d_spec; *row_stride = KG_SPEC_ROW;
    return KG_OK;
}

int kg_rxbank_fftext_set_rate(kg_rxbank *b, double sample_rate)
{
    KG_REQUIRE(b != nullptr, KG_ERR_INVALID, "kg_rxbank_fftext_set_rate: null argument");
    KG_REQUIRE(sample_rate > 0 && sample_rate <= 1e12, KG_ERR_INVALID, "kg_rxbank_fftext_set_rate: sample rate %g", sample_rate);
    if (b->fx.obj) KG_TRY(kg_fftext_set_rate(b->fx.obj, sample_rate));
    b->fx.rate = sample_rate;
    return KG_OK;
}

// `SET run=%d` (FFT.cpp:206-244): snd->isSAM and snd->mode == MODE_QAM are the bank's view of kg_post's mode NOW, as the reference reads them
int kg_rxbank_fftext_set_run(kg_rxbank *b, int rx, int run)
{
    KG_TRY(bank_rx_check(b, rx, "kg_rxbank_fftext_set_run"));
    KG_REQUIRE(run >= KG_FFTEXT_OFF && run <= KG_FFTEXT_INTEG, KG_ERR_INVALID, "kg_rxbank_fftext_set_run: run %d (-1..2)", run);      // (refused before anything is made)
    KG_TRY(bank_fx_ensure(b));
    const int mode = kg_post_get_mode(b->post, rx);
    KG_TRY(kg_fftext_set_run(b->fx.obj, rx, run, mode >= KG_POST_SAM && mode <= KG_POST_QAM, mode == KG_POST_QAM));
    b->fx.on[rx] = run != KG_FFTEXT_OFF;
    return KG_OK;
}

int kg_rxbank_fftext_set_itime(kg_rxbank *b, int rx, double itime) { BANK_EXT("kg_rxbank_fftext_set_itime", bank_fx_ensure); return kg_fftext_set_itime(b->fx.obj, rx, itime); }
int kg_rxbank_fftext_clear(kg_rxbank *b, int rx) { BANK_EXT("kg_rxbank_fftext_clear", bank_fx_ensure); return kg_fftext_clear(b->fx.obj, rx); }

kg_fftext *kg_rxbank_fftext(kg_rxbank *b) { return b ? b->fx.obj : nullptr; }

int kg_rxbank_fftext_max(kg_rxbank *b)
{
    KG_REQUIRE(b != nullptr, KG_ERR_INVALID, "kg_rxbank_fftext_max: null argument");
    return (int) b->fx.max;
}

int kg_rxbank_fftext_map(kg_rxbank *b, int32_t *rx_of_row, int32_t *blk_of_row, int32_t *bin_of_row)
{
    KG_REQUIRE(b != nullptr, KG_ERR_INVALID, "kg_rxbank_fftext_map: null argument");
    for (int r = 0; r < b->fx.last.n; r++) {
        if (rx_of_row) rx_of_row[r] = b->fx.last.rx[r];
        if (blk_of_row) blk_of_row[r] = b->fx.last.blk[r];
        if (bin_of_row) bin_of_row[r] = b->fx.last.bin[r];
    }
    return b->fx.last.n;
}

int kg_rxbank_fftext_rows(kg_rxbank *b, uint8_t **d_rows, size_t *row_stride)
{
    KG_REQUIRE(b && d_rows && row_stride, KG_ERR_INVALID, "kg_rxbank_fftext_rows: null argument");
    *d_rows = b->fx.d_rows; *row_stride = KG_FFTEXT_ROW;          // null until the extension was named
    return KG_OK;
}

int kg_rxbank_iqd_init(kg_rxbank *b, int rx)
{
    BANK_EXT("kg_rxbank_iqd_init", bank_iq_ensure);
    b->iq.on[rx] = 0;                                      // a fresh object is not registered
    return kg_iqd_init(b->iq.obj, rx);
}

int kg_rxbank_iqd_set_run(kg_rxbank *b, int rx, int run, double rate)
{
    BANK_EXT("kg_rxbank_iqd_set_run", bank_iq_ensure);
    if (run) KG_TRY(bank_tap_free(b, rx, "kg_rxbank_iqd_set_run", false));
    KG_TRY(kg_iqd_set_run(b->iq.obj, rx, run, rate));
    b->iq.on[rx] = run != 0;
    return KG_OK;
}

int kg_rxbank_iqd_set_gain(kg_rxbank *b, int rx, int gain) { BANK_EXT("kg_rxbank_iqd_set_gain", bank_iq_ensure); return kg_iqd_set_gain(b->iq.obj, rx, gain); }
int kg_rxbank_iqd_set_points(kg_rxbank *b, int rx, int points) { BANK_EXT("kg_rxbank_iqd_set_points", bank_iq_ensure); return kg_iqd_set_points(b->iq.obj, rx, points); }
int kg_rxbank_iqd_set_pll_mode(kg_rxbank *b, int rx, int pll_mode, int arg) { BANK_EXT("kg_rxbank_iqd_set_pll_mode", bank_iq_ensure); return kg_iqd_set_pll_mode(b->iq.obj, rx, pll_mode, arg); }
int kg_rxbank_iqd_set_pll_bandwidth(kg_rxbank *b, int rx, float bandwidth) { BANK_EXT("kg_rxbank_iqd_set_pll_bandwidth", bank_iq_ensure); return kg_iqd_set_pll_bandwidth(b->iq.obj, rx, bandwidth); }
int kg_rxbank_iqd_set_draw(kg_rxbank *b, int rx, int draw) { BANK_EXT("kg_rxbank_iqd_set_draw", bank_iq_ensure); return kg_iqd_set_draw(b->iq.obj, rx, draw); }
int kg_rxbank_iqd_set_display_mode(kg_rxbank *b, int rx, int display_mode) { BANK_EXT("kg_rxbank_iqd_set_display_mode", bank_iq_ensure); return kg_iqd_set_display_mode(b->iq.obj, rx, display_mode); }
int kg_rxbank_iqd_clear(kg_rxbank *b, int rx) { BANK_EXT("kg_rxbank_iqd_clear", bank_iq_ensure); return kg_iqd_clear(b->iq.obj, rx); }

kg_iqd *kg_rxbank_iqd(kg_rxbank *b) { return b ? b->iq.obj : nullptr; }

int kg_rxbank_iqd_map(kg_rxbank *b, kg_iqd_row *row_map, int max_rows)
{
    KG_REQUIRE(b != nullptr && max_rows >= 0, KG_ERR_INVALID, "kg_rxbank_iqd_map: bad argument");
    KG_REQUIRE(!row_map || max_rows >= b->iq.last.n, KG_ERR_INVALID, "kg_rxbank_iqd_map: %d rows, room for %d", b->iq.last.n, max_rows);
    if (row_map && b->iq.last.n) memcpy(row_map, b->iq.last.rows.data(), sizeof(kg_iqd_row) * (size_t) b->iq.last.n);
    return b->iq.last.n;
}

int kg_rxbank_iqd_rows(kg_rxbank *b, uint8_t **d_rows, size_t *rows_cap)
{
    KG_REQUIRE(b && d_rows && rows_cap, KG_ERR_INVALID, "kg_rxbank_iqd_rows: null argument");
    *d_rows = b->iq.d_rows; *rows_cap = b->iq.cap;                // null until the extension was named
    return KG_OK;
}

int kg_rxbank_iqd_status(kg_rxbank *b, kg_iqd_status **d_status, int32_t *rx_of_blk, int32_t *blk_of_blk, int32_t *sent_of_blk)
{
    KG_REQUIRE(b != nullptr, KG_ERR_INVALID, "kg_rxbank_iqd_status: null argument");
    if (d_status) *d_status = b->iq.d_st;
    for (int k = 0; k < b->iq.last.nblk; k++) {
        if (rx_of_blk) rx_of_blk[k] = b->iq.last.blk_rx[k];
        if (blk_of_blk) blk_of_blk[k] = b->iq.last.blk_blk[k];
        if (sent_of_blk) sent_of_blk[k] = b->iq.last.sent[k];
    }
    return b->iq.last.nblk;
}

int kg_rxbank_lorc_init(kg_rxbank *b, int rx, double srate, int i_srate) { BANK_EXT("kg_rxbank_lorc_init", bank_lo_ensure); return kg_lorc_init(b->lo.obj, rx, srate, i_srate); }
int kg_rxbank_lorc_set_gri(kg_rxbank *b, int rx, int ch, int gri) { BANK_EXT("kg_rxbank_lorc_set_gri", bank_lo_ensure); return kg_lorc_set_gri_min_(b->lo.obj, rx, ch, gri, BANK_LO_MIN_SPG); }
int kg_rxbank_lorc_set_offset(kg_rxbank *b, int rx, int ch, int offset) { BANK_EXT("kg_rxbank_lorc_set_offset", bank_lo_ensure); return kg_lorc_set_offset(b->lo.obj, rx, ch, offset); }
int kg_rxbank_lorc_set_gain(kg_rxbank *b, int rx, int ch, int gain) { BANK_EXT("kg_rxbank_lorc_set_gain", bank_lo_ensure); return kg_lorc_set_gain(b->lo.obj, rx, ch, gain); }
int kg_rxbank_lorc_set_avg_algo(kg_rxbank *b, int rx, int ch, int avg_algo) { BANK_EXT("kg_rxbank_lorc_set_avg_algo", bank_lo_ensure); return kg_lorc_set_avg_algo(b->lo.obj, rx, ch, avg_algo); }
int kg_rxbank_lorc_set_avg_param(kg_rxbank *b, int rx, int ch, double avg_param) { BANK_EXT("kg_rxbank_lorc_set_avg_param", bank_lo_ensure); return kg_lorc_set_avg_param(b->lo.obj, rx, ch, avg_param); }

int kg_rxbank_lorc_start(kg_rxbank *b, int rx)
{
    BANK_EXT("kg_rxbank_lorc_start", bank_lo_ensure);
    KG_TRY(bank_tap_free(b, rx, "kg_rxbank_lorc_start", true));
    KG_TRY(kg_lorc_start(b->lo.obj, rx));
    b->lo.on[rx] = 1;
    return KG_OK;
}

int kg_rxbank_lorc_stop(kg_rxbank *b, int rx)
{
    BANK_EXT("kg_rxbank_lorc_stop", bank_lo_ensure);
    KG_TRY(kg_lorc_stop(b->lo.obj, rx));
    b->lo.on[rx] = 0;
    return KG_OK;
}

kg_lorc *kg_rxbank_lorc(kg_rxbank *b) { return b ? b->lo.obj : nullptr; }

int kg_rxbank_lorc_map(kg_rxbank *b, kg_lorc_row *row_map, int max_rows)
{
    KG_REQUIRE(b != nullptr && max_rows >= 0, KG_ERR_INVALID, "kg_rxbank_lorc_map: bad argument");
    KG_REQUIRE(!row_map || max_rows >= b->lo.last.n, KG_ERR_INVALID, "kg_rxbank_lorc_map: %d rows, room for %d", b->lo.last.n, max_rows);
    if (row_map && b->lo.last.n) memcpy(row_map, b->lo.last.rows.data(), sizeof(kg_lorc_row) * (size_t) b->lo.last.n);
    return b->lo.last.n;
}

int kg_rxbank_lorc_rows(kg_rxbank *b, uint8_t **d_rows, size_t *cap)
{
    KG_REQUIRE(b && d_rows && cap, KG_ERR_INVALID, "kg_rxbank_lorc_rows: null argument");
    *d_rows = b->lo.d_rows; *cap = b->lo.cap;                     // null until the extension was named
    return KG_OK;
}

int kg_rxbank_fax_start(kg_rxbank *b, int rx, int lpm, int imagewidth, int carrier, int deviation, int bandwidth, int include_headers, int phasing, int autostop,
                        int debug, double nom_rate, double srate)
{
    BANK_EXT("kg_rxbank_fax_start", bank_fa_ensure);
    KG_TRY(bank_real_tap_free(b, rx, "kg_rxbank_fax_start", TAP_FAX));
    KG_REQUIRE(imagewidth <= BANK_FAX_MAX_WIDTH, KG_ERR_INVALID, "kg_rxbank_fax_start: imagewidth %d; a receiver bank takes %d or fewer", imagewidth,
               BANK_FAX_MAX_WIDTH);
    KG_REQUIRE(!(lpm >= 1 && nom_rate >= 1) || nom_rate * 60.0 / lpm >= BANK_FAX_MIN_SPL, KG_ERR_INVALID,
               "kg_rxbank_fax_start: %g samples a line; a receiver bank takes %d or more (it bounds a step's lines by it)", nom_rate * 60.0 / lpm, BANK_FAX_MIN_SPL);
    KG_TRY(kg_fax_start(b->fa.obj, rx, lpm, imagewidth, carrier, deviation, bandwidth, include_headers, phasing, autostop, debug, nom_rate, srate));
    b->fa.on[rx] = 1;
    b->fa.rate[rx] = srate;
    return KG_OK;
}

int kg_rxbank_fax_set_shift(kg_rxbank *b, int rx, float shift) { BANK_EXT("kg_rxbank_fax_set_shift", bank_fa_ensure); return kg_fax_set_shift(b->fa.obj, rx, shift); }

int kg_rxbank_fax_stop(kg_rxbank *b, int rx)
{
    BANK_EXT("kg_rxbank_fax_stop", bank_fa_ensure);
    KG_TRY(kg_fax_stop(b->fa.obj, rx));
    b->fa.on[rx] = 0;
    return KG_OK;
}

kg_fax *kg_rxbank_fax(kg_rxbank *b) { return b ? b->fa.obj : nullptr; }

int kg_rxbank_fax_out(kg_rxbank *b, uint8_t **d_rows, size_t *row_stride, kg_fax_rec **d_recs, int32_t **d_counts, int32_t *max_lines, int32_t *rx_of_entry,
                      int max_entries)
{
    KG_REQUIRE(b != nullptr && max_entries >= 0, KG_ERR_INVALID, "kg_rxbank_fax_out: bad argument");
    const bank_fa &x = b->fa;
    KG_REQUIRE(!rx_of_entry || max_entries >= x.last.n, KG_ERR_INVALID, "kg_rxbank_fax_out: %d entries, room for %d", x.last.n, max_entries);
    if (d_rows) *d_rows = x.d_rows;                                      // null until the extension was named
    if (row_stride) *row_stride = x.row_stride;
    if (d_recs) *d_recs = x.d_recs;
    if (d_counts) *d_counts = x.d_counts;
    if (max_lines) *max_lines = x.max_lines;
    if (rx_of_entry && x.last.n) memcpy(rx_of_entry, x.last.rx.data(), sizeof(int32_t) * (size_t) x.last.n);
    return x.last.n;
}

int kg_rxbank_cw_start(kg_rxbank *b, int rx, int training_interval, double nom_rate, double srate)
{
    BANK_EXT("kg_rxbank_cw_start", bank_cw_ensure);
    KG_TRY(bank_real_tap_free(b, rx, "kg_rxbank_cw_start", TAP_CW));
    KG_TRY(kg_cw_start(b->cw.obj, rx, training_interval, nom_rate, srate));
    b->cw.on[rx] = 1;
    return KG_OK;
}

int kg_rxbank_cw_set_wpm(kg_rxbank *b, int rx, int wpm, int training_interval)
{
    BANK_EXT("kg_rxbank_cw_set_wpm", bank_cw_ensure);
    return kg_cw_set_wpm(b->cw.obj, rx, wpm, training_interval);
}

int kg_rxbank_cw_set_pboff(kg_rxbank *b, int rx, uint32_t pboff) { BANK_EXT("kg_rxbank_cw_set_pboff", bank_cw_ensure); return kg_cw_set_pboff(b->cw.obj, rx, pboff); }

int kg_rxbank_cw_set_wsc(kg_rxbank *b, int rx, int wsc) { BANK_EXT("kg_rxbank_cw_set_wsc", bank_cw_ensure); return kg_cw_set_wsc(b->cw.obj, rx, wsc); }

int kg_rxbank_cw_set_auto_threshold(kg_rxbank *b, int rx, int on)
{
    BANK_EXT("kg_rxbank_cw_set_auto_threshold", bank_cw_ensure);
    return kg_cw_set_auto_threshold(b->cw.obj, rx, on);
}

int kg_rxbank_cw_set_threshold(kg_rxbank *b, int rx, int threshold)
{
    BANK_EXT("kg_rxbank_cw_set_threshold", bank_cw_ensure);
    return kg_cw_set_threshold(b->cw.obj, rx, threshold);
}

int kg_rxbank_cw_stop(kg_rxbank *b, int rx)
{
    BANK_EXT("kg_rxbank_cw_stop", bank_cw_ensure);
    KG_TRY(kg_cw_stop(b->cw.obj, rx));
    b->cw.on[rx] = 0;
    return KG_OK;
}

int kg_rxbank_cw_set_now(kg_rxbank *b, uint32_t now_sec)
{
    KG_REQUIRE(b != nullptr, KG_ERR_INVALID, "kg_rxbank_cw_set_now: null handle");
    b->cw.now = now_sec;                        // the plan of every later step copies it into the step's table
    return KG_OK;
}

kg_cw *kg_rxbank_cw(kg_rxbank *b) { return b ? b->cw.obj : nullptr; }

int kg_rxbank_wspr_init(kg_rxbank *b, int rx, double snd_rate) { BANK_EXT("kg_rxbank_wspr_init", bank_ws_ensure); return kg_wspr_init(b->ws.obj, rx, snd_rate); }

int kg_rxbank_wspr_set_capture(kg_rxbank *b, int rx, int capture)
{
    BANK_EXT("kg_rxbank_wspr_set_capture", bank_ws_ensure);
    if (capture) KG_TRY(bank_tap_free_for_wspr(b, rx, "kg_rxbank_wspr_set_capture"));
    KG_TRY(kg_wspr_set_capture(b->ws.obj, rx, capture));
    b->ws.on[rx] = capture ? 1 : 0;
    return KG_OK;
}

int kg_rxbank_wspr_set_type(kg_rxbank *b, int rx, int type) { BANK_EXT("kg_rxbank_wspr_set_type", bank_ws_ensure); return kg_wspr_set_type(b->ws.obj, rx, type); }

int kg_rxbank_wspr_set_more_candidates(kg_rxbank *b, int rx, int on)
{
    BANK_EXT("kg_rxbank_wspr_set_more_candidates", bank_ws_ensure);
    return kg_wspr_set_more_candidates(b->ws.obj, rx, on);
}

int kg_rxbank_wspr_set_now(kg_rxbank *b, int minute, int second)
{
    KG_REQUIRE(b != nullptr, KG_ERR_INVALID, "kg_rxbank_wspr_set_now: null handle");
    KG_REQUIRE(minute >= 0 && minute <= 59 && second >= 0 && second <= 59, KG_ERR_INVALID, "kg_rxbank_wspr_set_now: %d:%d (0..59 each)", minute, second);
    b->ws.min = minute; b->ws.sec = second;     // the plan of every later step copies them into the step's table
    return KG_OK;
}

kg_wspr *kg_rxbank_wspr(kg_rxbank *b) { return b ? b->ws.obj : nullptr; }

int kg_rxbank_wspr_out(kg_rxbank *b, uint8_t **d_rows, kg_wspr_cycle **d_cycles, int32_t **d_counts, kg_wspr_row *row_map, int max_rows, int32_t *nrows,
                       kg_wspr_ev *evs, int max_events, int32_t *nevents, int32_t *rx_of_entry, int max_entries)
{
    KG_REQUIRE(b != nullptr && max_rows >= 0 && max_events >= 0 && max_entries >= 0, KG_ERR_INVALID, "kg_rxbank_wspr_out: bad argument");
    const bank_ws &x = b->ws;
    KG_REQUIRE(!row_map || max_rows >= x.last.n, KG_ERR_INVALID, "kg_rxbank_wspr_out: %d rows, room for %d", x.last.n, max_rows);
    KG_REQUIRE(!evs || max_events >= x.last.ne, KG_ERR_INVALID, "kg_rxbank_wspr_out: %d events, room for %d", x.last.ne, max_events);
    KG_REQUIRE(!rx_of_entry || max_entries >= x.last.nent, KG_ERR_INVALID, "kg_rxbank_wspr_out: %d entries, room for %d", x.last.nent, max_entries);
    if (d_rows) *d_rows = x.d_rows.p;
    if (d_cycles) *d_cycles = x.d_cycles.p;
    if (d_counts) *d_counts = x.d_counts.p;
    if (row_map && x.last.n) memcpy(row_map, x.last.rows.data(), sizeof(kg_wspr_row) * (size_t) x.last.n);
    if (evs && x.last.ne) memcpy(evs, x.last.evs.data(), sizeof(kg_wspr_ev) * (size_t) x.last.ne);
    if (nrows) *nrows = x.last.n;
    if (nevents) *nevents = x.last.ne;
    for (int e = 0; rx_of_entry && e < x.last.nent; e++) rx_of_entry[e] = x.last.rx[e];
    return x.last.nent;
}

// ---- WSPR stage 2: the table, pass 0 behind a step's cycle end, its records
int kg_rxbank_wspr_set_metric_table(kg_rxbank *b, const int32_t mettab[2][256])
{
    KG_REQUIRE(b != nullptr, KG_ERR_INVALID, "kg_rxbank_wspr_set_metric_table: null handle");
    KG_TRY(bank_ws_ensure(b));
    return kg_wspr_set_metric_table(b->ws.obj, mettab);
}

int kg_rxbank_wspr_set_decode(kg_rxbank *b, int rx, int on) { BANK_EXT("kg_rxbank_wspr_set_decode", bank_ws_ensure); return kg_wspr_set_decode(b->ws.obj, rx, on); }

int kg_rxbank_wspr_dec_out(kg_rxbank *b, kg_wspr_dec **d_decs, int32_t **d_ncand, int32_t *rx_decoded, int max_rx)
{
    KG_REQUIRE(b != nullptr && max_rx >= 0, KG_ERR_INVALID, "kg_rxbank_wspr_dec_out: bad argument");
    const bank_ws &x = b->ws;
    if (d_decs) *d_decs = nullptr;
    if (d_ncand) *d_ncand = nullptr;
    if (!x.obj) return 0;                                               // never told
    kg_wspr_dec *dd = nullptr;
    int32_t *dn = nullptr;
    kg_wspr_dec_buffers_(x.obj, &dd, &dn);
    if (d_decs) *d_decs = dd;
    if (d_ncand) *d_ncand = dn;
    int n = 0;
    for (int e = 0; e < x.last.ne; e++)
        if (x.last.evs[e].kind == KG_WSPR_EV_DECODES) {
            KG_REQUIRE(!rx_decoded || n < max_rx, KG_ERR_INVALID, "kg_rxbank_wspr_dec_out: more than %d receivers decoded", max_rx);
            if (rx_decoded) rx_decoded[n] = x.last.evs[e].conn;
            n++;
        }
    return n;
}

// ---- FT8 / FT4 (include/kiwigpu_ft8.h)
int kg_rxbank_ft8_init(kg_rxbank *b, int rx, int protocol, double snd_rate)
{
    BANK_EXT("kg_rxbank_ft8_init", bank_f8_ensure);
    return kg_ft8_init(b->f8.obj, rx, protocol, snd_rate);
}

int kg_rxbank_ft8_start(kg_rxbank *b, int rx)
{
    BANK_EXT("kg_rxbank_ft8_start", bank_f8_ensure);
    KG_TRY(bank_real_tap_free(b, rx, "kg_rxbank_ft8_start", TAP_FT8));
    KG_REQUIRE(kg_ft8_inited_(b->f8.obj, rx), KG_ERR_STATE, "kg_rxbank_ft8_start: receiver %d was never initialised (kg_rxbank_ft8_init)", rx);
    b->f8.on[rx] = 1;
    return KG_OK;
}

int kg_rxbank_ft8_stop(kg_rxbank *b, int rx)
{
    KG_TRY(bank_rx_check(b, rx, "kg_rxbank_ft8_stop"));
    b->f8.on[rx] = 0;                           // a bank that was never told has nothing to stop, and makes nothing for it
    return KG_OK;
}

int kg_rxbank_ft8_set_now(kg_rxbank *b, double now)
{
    KG_REQUIRE(b != nullptr, KG_ERR_INVALID, "kg_rxbank_ft8_set_now: null handle");
    KG_REQUIRE(now >= 0.0 && now <= 1099511627776.0, KG_ERR_INVALID, "kg_rxbank_ft8_set_now: time %g (finite, 0 .. 2^40)", now);
    b->f8.now = now;                            // the plan of every later step copies it into the step's callbacks
    return KG_OK;
}

kg_ft8 *kg_rxbank_ft8(kg_rxbank *b) { return b ? b->f8.obj : nullptr; }

int kg_rxbank_ft8_out(kg_rxbank *b, kg_ft8_slot **d_slots, kg_ft8_ev *evs, int max_events, int32_t *nevents, int32_t *rx_of_slot, int max_slots)
{
    KG_REQUIRE(b != nullptr && max_events >= 0 && max_slots >= 0, KG_ERR_INVALID, "kg_rxbank_ft8_out: bad argument");
    const bank_f8 &x = b->f8;
    KG_REQUIRE(!evs || max_events >= x.last.ne, KG_ERR_INVALID, "kg_rxbank_ft8_out: %d events, room for %d", x.last.ne, max_events);
    KG_REQUIRE(!rx_of_slot || max_slots >= x.last.nsl, KG_ERR_INVALID, "kg_rxbank_ft8_out: %d slot records, room for %d", x.last.nsl, max_slots);
    if (d_slots) *d_slots = x.d_slots;                                  // null until the extension was named
    if (evs && x.last.ne) memcpy(evs, x.last.evs.data(), sizeof(kg_ft8_ev) * (size_t) x.last.ne);
    if (nevents) *nevents = x.last.ne;
    if (rx_of_slot && x.last.nsl) memcpy(rx_of_slot, x.last.slot_rx.data(), sizeof(int32_t) * (size_t) x.last.nsl);
    return x.last.nsl;
}

int kg_rxbank_cw_out(kg_rxbank *b, kg_cw_ev **d_evs, int32_t **d_counts, int32_t *max_events, int32_t *rx_of_entry, int max_entries)
{
    KG_REQUIRE(b != nullptr && max_entries >= 0, KG_ERR_INVALID, "kg_rxbank_cw_out: bad argument");
    const bank_cw &x = b->cw;
    KG_REQUIRE(!rx_of_entry || max_entries >= x.last.n, KG_ERR_INVALID, "kg_rxbank_cw_out: %d entries, room for %d", x.last.n, max_entries);
    if (d_evs) *d_evs = x.d_evs;                                        // null until the extension was named
    if (d_counts) *d_counts = x.d_counts;
    if (max_events) *max_events = x.max_events;
    if (rx_of_entry && x.last.n) memcpy(rx_of_entry, x.last.rx.data(), sizeof(int32_t) * (size_t) x.last.n);
    return x.last.n;
}

int kg_rxbank_set_wf(kg_rxbank *b, int rx, uint64_t phase_inc, int decim, int overlapped)
{
    KG_TRY(bank_rx_check(b, rx, "kg_rxbank_set_wf"));
    KG_REQUIRE(decim >= 1 && (decim & (decim - 1)) == 0 && decim <= 8192, KG_ERR_INVALID, "kg_rxbank_set_wf: decimation %d", decim);
    if (overlapped) {
        const size_t m = b->n / (size_t) decim;
        // (m even: a frame is read at ring offset w + m - 8192, and kg_wf_frames_at_dev takes 8-byte aligned frames)
        KG_REQUIRE(b->n % (size_t) decim == 0 && m >= 2 && m <= KG_WF_NFFT && KG_WF_NFFT % m == 0, KG_ERR_INVALID,
                   "kg_rxbank_set_wf: overlapped sampling needs a step (%zu samples) that yields an even divisor of 8192 outputs at R = %d "
                   "(a faster sampler fills a frame per step: use the one-shot mode)", b->n, decim);
    } else {
        KG_REQUIRE((size_t) KG_WF_NFFT * (size_t) decim <= b->n, KG_ERR_INVALID,
                   "kg_rxbank_set_wf: a one-shot frame at R = %d takes %zu samples, a step has %zu: use the overlapped mode "
                   "(rx_waterfall.cpp:967-983)", decim, (size_t) KG_WF_NFFT * (size_t) decim, b->n);
    }
    KG_TRY(bank_drain(b, false));
    int rc = kg_ddc_set_wf(b->ddc, rx, phase_inc, decim);
    if (rc) return rc;
    bank_rx &r = b->rcv[rx];
    if (r.wf_set && decim != r.decim) bank_nb_zoom_change(b, rx);
    r.decim = decim; r.overlapped = overlapped ? 1 : 0; r.wf_set = 1;
    r.ring_w = 0; r.ring_total = 0;                        // CmdWFReset: the sampler starts empty ("fill pipe")
    return KG_OK;
}

// A connection ends: the receiver is left out of every stage from the next step on (its state stays where it is).
int kg_rxbank_leave(kg_rxbank *b, int rx)
{
    KG_TRY(bank_rx_check(b, rx, "kg_rxbank_leave"));
    b->rcv[rx].active = 0;
    return bank_ext_fresh(b, rx);
}

// A connection starts on receiver rx (rx/rx_sound.cpp:236-269, rx/rx_waterfall.cpp:205-330): its audio DDC, CFastFIR position,
// S-meter / detector state, ADPCM state and sound sequence number start from zero, its waterfall sampler is empty and waits for
// kg_rxbank_set_wf; no other receiver is touched (their DDC counters, FIR positions and sequence numbers run on -- from here
// on this receiver's sound blocks complete on its OWN steps).  The host then configures it through the per-seam objects
// (kg_rxddc_set_freq, kg_fir_setup, kg_post_*) as for a fresh bank.  Drains the bank's streams.
int kg_rxbank_join(kg_rxbank *b, int rx)
{
    KG_TRY(bank_rx_check(b, rx, "kg_rxbank_join"));
    KG_HIP(hipSetDevice(b->device));
    KG_TRY(bank_drain(b, true));
    KG_TRY(kg_rxddc_reset(b->rx, rx));
    KG_TRY(kg_fir_reset(b->fir, rx));
    KG_TRY(kg_fir_reset(b->nullfir, rx));
    KG_TRY(kg_post_reset(b->post, rx));
    KG_TRY(kg_adpcm_set_state(b->adpcm, rx, 0, 0));
    KG_TRY(bank_drain(b, false));
    bank_rx &r = b->rcv[rx];
    // the connection's fields, in bank_rx's order (the settings below them stay)
    r.snd_seq = 0; r.last_nrec = 0; r.last_nfir = 0;
    r.wf_set = 0; r.ring_w = 0; r.ring_total = 0;
    r.spec_on = 0; kg_spec::emit_clear(r.spec_mirror);     // memset(snd_t): specAF_FFT NULL, isChanNull false
    r.spec_cmds = kg_post_mode_cmds_(b->post, rx);
    KG_TRY(bank_ext_fresh(b, rx));                         // the extensions' state is the connection's
    r.nbc = bank_nb_cmd{};                                 // memset(snd_t) / memset(wf_inst_t): algo NB_OFF, enables and params 0;
    KG_TRY(kg_wf_set_nb(b->wf, rx, 0));                    // the blankers' states stay (the reference's CNoiseProc arrays are globals)
    r.active = 1;
    return KG_OK;
}

int kg_rxbank_is_active(kg_rxbank *b, int rx)
{
    KG_TRY(bank_rx_check(b, rx, "kg_rxbank_is_active"));
    return b->rcv[rx].active ? 1 : 0;
}

// Per receiver, after the last step (arrays of nrx entries, any may be NULL): rx_iq_t records and CFastFIR outputs the step gave
// it (0 for a receiver that is not active), FirPos() now, sound blocks it has emitted since it joined (= the seq its next
// packets carry).
int kg_rxbank_audio_map(kg_rxbank *b, int32_t *nrec, int32_t *nfir, int32_t *fir_pos, uint32_t *snd_seq)
{
    KG_REQUIRE(b != nullptr, KG_ERR_INVALID, "kg_rxbank_audio_map: null argument");
    for (int k = 0; k < b->nrx; k++) {
        if (nrec) nrec[k] = b->rcv[k].last_nrec;
        if (nfir) nfir[k] = b->rcv[k].last_nfir;
        if (fir_pos) fir_pos[k] = kg_fir_pos(b->fir, k);
        if (snd_seq) snd_seq[k] = b->rcv[k].snd_seq;
    }
    return KG_OK;
}

int kg_rxbank_set_little_endian(kg_rxbank *b, int rx, int little_endian)
{
    KG_TRY(bank_rx_check(b, rx, "kg_rxbank_set_little_endian"));
    b->rcv[rx].little_endian = little_endian ? 1 : 0;
    return KG_OK;
}

int kg_rxbank_set_unpack(kg_rxbank *b, float rescale, float dc_i, float dc_q, int spectral_inversion)
{
    KG_REQUIRE(b != nullptr, KG_ERR_INVALID, "kg_rxbank_set_unpack: null argument");
    b->rescale = rescale; b->dc_i = dc_i; b->dc_q = dc_q; b->spectral_inversion = spectral_inversion ? 1 : 0;
    return KG_OK;
}

int kg_rxbank_set_wf_pkt(kg_rxbank *b, int rx, uint32_t x_bin_server, uint32_t zoom, int use_compression)
{
    KG_TRY(bank_rx_check(b, rx, "kg_rxbank_set_wf_pkt"));
    kg_wf_pkt_info &pkt = b->rcv[rx].pkt;
    if (zoom != pkt.zoom) bank_nb_zoom_change(b, rx);
    pkt.x_bin_server = x_bin_server; pkt.zoom = zoom; pkt.use_compression = use_compression ? 1 : 0;
    return KG_OK;
}

// rx_waterfall.cpp:1087-1096: a pending parameter change is set up before the receiver's next frame, once both enables are on
static int bank_wf_nb_pending(kg_rxbank *b)
{
    for (int k = 0; k < b->nrx; k++) {
        if (!b->rcv[k].active) continue;
        bank_nb_cmd &c = b->rcv[k].nbc;
        const bool both = c.wf_en[KG_NB_BLANKER] && c.wf_en[KG_NB_WF];
        if (both && c.wf_change[KG_NB_BLANKER]) {
            KG_TRY(kg_wf_nb_setup(b->wf, k, c.wf_param[KG_NB_BLANKER]));
            c.wf_change[KG_NB_BLANKER] = 0;
            c.wf_setup = 1;
        }
        KG_TRY(kg_wf_set_nb(b->wf, k, both && c.wf_setup));
    }
    return KG_OK;
}

// the ONE transfer of the step, on a stream of its own (ordered behind nothing but earlier uploads: the slot is free)
static int bank_upload(kg_rxbank *b, void *adc_ready_event)
{
    const kg_arena &a = b->arena;
    hipStream_t us = b->s_up;
    if (const char *ev = kg_tuning_env("KIWIGPU_BANK_UPLOAD")) us = ev[0] == 'm' ? b->s_main : (ev[0] == 's' ? b->s_side : b->s_up);
    hipError_t e = hipMemcpyAsync(a.d_base, a.h_base, a.used, hipMemcpyHostToDevice, us);
    if (e == hipSuccess) e = hipEventRecord(b->ev_tab, us);
    if (e == hipSuccess && us != b->s_main) e = hipStreamWaitEvent(b->s_main, b->ev_tab, 0);
    if (e == hipSuccess && us != b->s_side) e = hipStreamWaitEvent(b->s_side, b->ev_tab, 0);
    if (e == hipSuccess && adc_ready_event) {
        e = hipStreamWaitEvent(b->s_main, (hipEvent_t) adc_ready_event, 0);
        if (e == hipSuccess) e = hipStreamWaitEvent(b->s_side, (hipEvent_t) adc_ready_event, 0);
    }
    if (e != hipSuccess) { kg_set_error("kg_rxbank_step: %s", hipGetErrorString(e)); return KG_ERR_HIP; }
    return KG_OK;
}

int kg_rxbank_step(kg_rxbank *b, const void *d_adc, void *adc_ready_event, kg_rxbank_step_info *info)
{
    KG_REQUIRE(b && d_adc, KG_ERR_INVALID, "kg_rxbank_step: null argument");
    KG_HIP(hipSetDevice(b->device));
    bank_tick tk;
    const int slot = (int) (b->step % BANK_SLOTS);
    if (b->ev_end_rec[slot])                               // the step that last used this slot (BANK_SLOTS steps ago) has run
        for (int j = 0; j < 3; j++) KG_HIP(hipEventSynchronize(b->ev_end[slot][j]));
    kg_arena &a = b->arena;
    a.h_base = b->h_slots + (size_t) slot * b->slot_bytes; a.d_base = b->d_slots + (size_t) slot * b->slot_bytes;
    a.cap = b->slot_bytes; a.used = 0; a.nent = 0; a.cursor = 0;
    tk.lap(b, PF_UPLOAD, true);
    KG_TRY(bank_wf_nb_pending(b));
    bank_plan_step(b);
    bank_set_arena(b, KG_ARENA_PLAN);
    int rc = bank_pass(b, d_adc);
    tk.lap(b, PF_PLAN, true);
    if (rc == KG_OK) rc = bank_upload(b, adc_ready_event);
    tk.lap(b, PF_UPLOAD, true);
    if (rc == KG_OK) {
        a.mode = KG_ARENA_REPLAY;
        rc = bank_pass(b, d_adc);
        if (rc == KG_OK && a.cursor != a.nent) { kg_set_error("kg_rxbank_step: %d of %d planned tables replayed", a.cursor, a.nent); rc = KG_ERR_STATE; }
    }
    bank_set_arena(b, KG_ARENA_OFF);
    if (rc) return rc;
    bank_commit(b);
    tk = bank_tick();
    KG_HIP(hipEventRecord(b->ev_end[slot][0], b->s_main));
    KG_HIP(hipEventRecord(b->ev_end[slot][1], b->s_side));
    KG_HIP(hipEventRecord(b->ev_end[slot][2], b->s_tail));
    b->ev_end_rec[slot] = true;
    tk.lap(b, PF_END, true);
    b->prof_steps++;
    b->step++;
    if (info) *info = b->last;
    return KG_OK;
}

// `stream` waits until the readers (both DDCs) of the ADC block of the step `steps_back` steps ago are done -- 1: the last
// step, 2: the one before it (the buffer a double-buffered ADC ring is about to refill), ... up to BANK_SLOTS.  The caller's
// writer of that buffer goes behind this.
int kg_rxbank_adc_done(kg_rxbank *b, void *stream, int steps_back)
{
    KG_REQUIRE(b && stream, KG_ERR_INVALID, "kg_rxbank_adc_done: null argument");
    KG_REQUIRE(steps_back >= 1 && steps_back <= BANK_SLOTS, KG_ERR_INVALID, "kg_rxbank_adc_done: steps_back %d (1..%d)", steps_back, BANK_SLOTS);
    if (b->step < (uint64_t) steps_back) return KG_OK;      // no such step yet: nothing has read the buffer
    const int slot = (int) ((b->step - (uint64_t) steps_back) % BANK_SLOTS);
    KG_HIP(hipStreamWaitEvent((hipStream_t) stream, b->ev_end[slot][0], 0));
    KG_HIP(hipStreamWaitEvent((hipStream_t) stream, b->ev_end[slot][1], 0));
    return KG_OK;
}

// 1: the next kg_rxbank_step will not wait (the step that last used its table slot, BANK_SLOTS steps ago, has run); 0: it would
// block until then -- a cooperative host (the reference's coroutine server) yields and asks again (NextTask in the data pump).
int kg_rxbank_ready(kg_rxbank *b)
{
    KG_REQUIRE(b != nullptr, KG_ERR_INVALID, "kg_rxbank_ready: null argument");
    KG_HIP(hipSetDevice(b->device));
    const int slot = (int) (b->step % BANK_SLOTS);
    if (!b->ev_end_rec[slot]) return 1;
    for (int j = 0; j < 3; j++) {
        const hipError_t e = hipEventQuery(b->ev_end[slot][j]);
        if (e == hipErrorNotReady) return 0;
        if (e != hipSuccess) { kg_set_error("kg_rxbank_ready: %s", hipGetErrorString(e)); return KG_ERR_HIP; }
    }
    return 1;
}

int kg_rxbank_poll(kg_rxbank *b)
{
    KG_REQUIRE(b != nullptr, KG_ERR_INVALID, "kg_rxbank_poll: null argument");
    KG_HIP(hipSetDevice(b->device));
    for (hipStream_t s : {b->s_main, b->s_side, b->s_tail}) {
        const hipError_t e = hipStreamQuery(s);
        if (e == hipErrorNotReady) return 0;
        if (e != hipSuccess) { kg_set_error("kg_rxbank_poll: %s", hipGetErrorString(e)); return KG_ERR_HIP; }
    }
    return 1;
}

int kg_rxbank_sync(kg_rxbank *b)
{
    KG_REQUIRE(b != nullptr, KG_ERR_INVALID, "kg_rxbank_sync: null argument");
    KG_HIP(hipSetDevice(b->device));
    return bank_drain(b, true);
}

// The host's share of the steps since the last call (or since create), by phase: text into buf.  The slot wait is where a
// host that runs ahead of the GPU blocks (BANK_SLOTS steps deep), so measure with the bank drained between steps.
int kg_rxbank_host_profile(kg_rxbank *b, char *buf, size_t len)
{
    KG_REQUIRE(b && buf && len > 0, KG_ERR_INVALID, "kg_rxbank_host_profile: null argument");
    size_t at = 0;
    double tot = 0;
    const double n = b->prof_steps ? (double) b->prof_steps : 1.0;
    for (int k = 0; k < PF_N; k++) tot += b->prof[k];
    at += (size_t) snprintf(buf + at, len - at, "%llu steps, %.1f us of host time per step:", (unsigned long long) b->prof_steps, tot / n * 1e6);
    for (int k = 0; k < PF_N && at < len; k++) at += (size_t) snprintf(buf + at, len - at, " %s %.1f;", PF_NAME[k], b->prof[k] / n * 1e6);
    for (int k = 0; k < PF_N; k++) b->prof[k] = 0;
    b->prof_steps = 0;
    return KG_OK;
}

int kg_rxbank_buffers(kg_rxbank *b, kg_rxbank_bufs *out)
{
    KG_REQUIRE(b && out, KG_ERR_INVALID, "kg_rxbank_buffers: null argument");
    out->wf_iq = b->d_wfiq; out->wf_iq_stride = b->wf_stride;
    out->wf_rows = b->d_rows; out->wf_pkts = b->d_pkts; out->wf_pkt_stride = BANK_PKT_STRIDE;
    out->rx_raw = b->d_raw; out->rx_stride = b->nrec_max;
    out->rx_in = b->d_xin;
    out->fir_out = b->d_firo; out->fir_stride = b->firo_stride;
    out->s16 = b->d_s16; out->adpcm = b->d_pay; out->agc = b->d_agc; out->iq_pay = b->d_iqpay;
    return KG_OK;
}

int kg_rxbank_frame_map(kg_rxbank *b, int32_t *rx_of_frame, uint64_t *frame_off, int32_t *pkt_bytes)
{
    KG_REQUIRE(b != nullptr, KG_ERR_INVALID, "kg_rxbank_frame_map: null argument");
    for (int f = 0; f < b->last.nframes; f++) {
        if (rx_of_frame) rx_of_frame[f] = b->frame_rx[f];
        if (frame_off) frame_off[f] = b->frame_off[f];
        if (pkt_bytes) pkt_bytes[f] = b->pkt_bytes[f];
    }
    return b->last.nframes;
}

}  // extern "C"
