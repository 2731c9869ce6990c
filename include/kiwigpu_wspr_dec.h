/* kiwigpu_wspr_dec.h -- the WSPR extension, stage 2 (extensions/wspr/wspr.cpp:45-212, :733-883, fano.cpp, wspr_util.cpp:208-230): from
 * a candidate of stage 1 to the 50 message bits.  Included by kiwigpu.h behind the stage-1 declarations (kg_wspr, kg_wspr_cand); a host
 * includes kiwigpu.h alone.
 *
 * One call is ONE pass of wspr_decode's candidate loop (:733-883, without unpk_ and what follows it) over the candidates a connection
 * holds: those of its last cycle end (kg_wspr_push, kg_wspr_load), or the ones kg_wspr_load_iq handed in.  Per candidate, in SNR order:
 * the six refinement calls of sync_and_demodulate (:759-805), the minsync1 gate (:795), the jiggle loop (:819-867) with soft symbols,
 * the rms / sync gate (:838), deinterleave and the Fano decoder, and the result classes (:869-883).  The object keeps p->ignore per
 * candidate across calls, set exactly where the reference sets it (:807, :875, :883): a later call skips those candidates (:740).  The
 * policy of passes is the caller's: the reference runs maxcycles 200 with iifac 2, then 1000, 5000, 10000 with iifac 1.  The tuning
 * constants of :505-513 are fixed: minsync1 0.10, minsync2 0.12, jig_range 128, symfac 50, delta 60, minrms 52 * (50 / 64.0).
 * csrc/kg_wspr_dec.h is the one definition for device and host, in the reference's operand types, and cites the reference item by item.
 *
 * THE SEEDS of the phase recurrences (:96-110), cos and sin in double of a float-valued phase step, are the CORRECTLY ROUNDED values
 * (csrc/kg_libm_dtrig.h), not the host libm's: results do not depend on the libm a host carries.  On the golden's scenes the reference
 * built either way gives the same records bit for bit (profiles/wspr_decode_golden.txt).
 * THE METRIC TABLE IS AN INPUT, as the clock is in stage 1: mettab[0][i] = round(10 * (t[i] - 0.45)), mettab[1][i] = mettab[0][255 - i]
 * for the caller's table t (:435-441).
 * THE RECORD IS THE SEQUENTIAL LOOP'S: the device evaluates all jiggles of a candidate at once, and reports what the reference's loop
 * over idt = 0, 1, 2 ... (ii = 0, -1, +1, -2, +2 ... times iifac, :820-822) would have left when it stopped at the first idt whose
 * gate passed and whose Fano run succeeded.
 * Defined here where the reference leaves it open: silence (totp 0) returns frequency 0.0, shift 0 and sync -1e30 from every search
 * call, to the letter; a NaN soft symbol is byte 0; Fano's nodes start as zeros; metric / cycles / maxnp / decdata are those of the
 * candidate's last Fano run, zeros if none ran; quickmode's single jiggle without a decode is KG_WSPR_QUICK_MISS.
 * REFUSED, nothing changed: a decode or kg_wspr_fano before the table is set (KG_ERR_STATE); iifac outside 1 .. 128; maxcycles outside
 * 1 .. 2^20; a table entry beyond +-2^20; a candidate handed in with |freq0| > 113, |shift0| > 45000 or |drift0| > 4; a connection
 * never initialised (KG_ERR_STATE) or listed twice. */
#ifndef KIWIGPU_WSPR_DEC_H
#define KIWIGPU_WSPR_DEC_H

enum { KG_WSPR_EV_DECODES = 2 };           /* kg_wspr_ev.kind behind KG_WSPR_EV_PEAKS: pass 0 of the cycle end was enqueued; a the decode half */
enum { KG_WSPR_SKIPPED = 0, KG_WSPR_MINSYNC1 = 1, KG_WSPR_NO_CHANGE = 2, KG_WSPR_TIME_UP = 3, KG_WSPR_DECODED = 4, KG_WSPR_QUICK_MISS = 5 };
typedef struct kg_wspr_dec {               /* one candidate of one pass, SNR order; all zeros behind the connection's last candidate */
    int32_t result;                        /* KG_WSPR_SKIPPED (ignore was set, :740), _MINSYNC1 (:795), _NO_CHANGE (time up and too weak, :873), _TIME_UP, _DECODED, _QUICK_MISS */
    int32_t ignore;                        /* the flag after this pass */
    float f1; int32_t shift1; float drift1, sync1;
    float tr_f[6]; int32_t tr_shift[6]; float tr_sync[6];      /* after each of the six refinement calls (the third and fourth: syncp, syncm); unreached calls 0 */
    int32_t idt, ii, jig_shift, gates; float rms;              /* the jiggles run, the last one's ii and shift, how many passed the gate, the last one's rms */
    uint32_t metric, cycles, maxnp;
    uint8_t decdata[11], symbols[162], pad[3];                 /* symbols: the last jiggle's, deinterleaved if it passed the gate */
} kg_wspr_dec;

/* mettab of wspr_init (:431-441) for the whole object: int32 [2][256], entries within +-2^20.  Synchronises. */
int kg_wspr_set_metric_table(kg_wspr *q, const int32_t mettab[2][256]);
/* The test and drop-in path, as kg_wspr_load is for planes: i_data / q_data [45000] each (wspr.h:224) into a half of connection conn,
 * which stage 2 decodes from until the connection's next cycle end (the schedule of kg_wspr_push is not touched), and cands [ncand <= 12] (freq0, shift0, drift0, sync0 of wspr.cpp:745-749; freq_idx and bin0 kept) as
 * its held candidates, SNR order, ignore cleared.  Synchronises. */
int kg_wspr_load_iq(kg_wspr *q, int conn, int half, const float *i_data, const float *q_data, const kg_wspr_cand *cands, int ncand);
/* One pass of wspr.cpp:733-883 on the decode half and held candidates of every listed connection (each at most once): maxcycles per
 * bit (fano.cpp:154), iifac (:508), quickmode (:866).  out [nconn][12] records, ncand [nconn] how many of them are candidates.  A
 * chain of launches on the context's stream with no host read between them; synchronises at the end. */
int kg_wspr_decode(kg_wspr *q, const int32_t *conns, int nconn, uint32_t maxcycles, int iifac, int quickmode, kg_wspr_dec *out, int32_t *ncand);
/* The Fano kernel alone (fano.cpp:91-244, delta 60) on n <= 4096 DEINTERLEAVED symbol sets [n][162]: per set fano's return value, metric,
 * cycles, maxnp and the 10 data bytes [n][10].  Synchronises. */
int kg_wspr_fano(kg_wspr *q, const uint8_t *symbols, int n, uint32_t maxcycles, int32_t *ok, uint32_t *metric, uint32_t *cycles, uint32_t *maxnp,
                 uint8_t *data);
/* When on, a cycle end inside kg_wspr_push also runs pass 0 of wspr.cpp:733-883 (maxcycles 200, iifac 2: :505, :508) on that
 * connection, enqueued behind the cycle-end launch with no host wait, and announces it by an event of kind KG_WSPR_EV_DECODES between
 * PEAKS and the resume.  Needs the table (KG_ERR_STATE); sizes the decode workspace for every connection of the object, so that a push
 * allocates nothing.  Off is the default, and then kg_wspr_push does exactly what it did before this call existed. */
int kg_wspr_set_decode(kg_wspr *q, int conn, int on);
/* The records [12] and the candidate count of the last pass 0 that a push ran for connection conn (wspr.cpp:733-883); zeros before the
 * first.  Later passes are kg_wspr_decode's.  Synchronises. */
int kg_wspr_decodes(kg_wspr *q, int conn, kg_wspr_dec *out, int32_t *ncand);

/* The receiver bank (kg_rxbank above in kiwigpu.h).  The table of wspr_init (wspr.cpp:431-441) for the bank's kg_wspr object: */
int kg_rxbank_wspr_set_metric_table(struct kg_rxbank *bank, const int32_t mettab[2][256]);
/* kg_wspr_set_decode for receiver rx: a step that holds its cycle end enqueues pass 0 (wspr.cpp:733-883) behind the cycle-end launch on
 * the tail stream, ahead of the step's end, with no host wait; the step's events carry KG_WSPR_EV_DECODES.  A step without a cycle end
 * launches nothing new; a bank never told is the bank it was.  Later passes are the host's: kg_wspr_decode on kg_rxbank_wspr(bank)
 * between steps, after kg_rxbank_sync. */
int kg_rxbank_wspr_set_decode(struct kg_rxbank *bank, int rx, int on);
/* The records of pass 0 (wspr.cpp:733-883) by receiver, device memory of the bank valid until its end: d_decs [nrx][12], d_ncand [nrx]
 * (NULL both for a bank never told); rx_decoded: the receivers whose pass 0 the LAST step enqueued.  Returns how many. */
int kg_rxbank_wspr_dec_out(struct kg_rxbank *bank, kg_wspr_dec **d_decs, int32_t **d_ncand, int32_t *rx_decoded, int max_rx);

#endif
