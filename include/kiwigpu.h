/*
 * kiwigpu.h -- C ABI of libkiwigpu.so: the MI355X (gfx950) implementation of
 * the FlyDog_SDR_GPS DSP hot path.
 *
 * The reference has no FFI seam for this path; the seam is function-level
 * inside the kiwid process.  Every entry point below
 * names the reference function(s) it replaces (file:line under the reference
 * tree).  INTEGRATION.md shows the binding a maintainer adds on the reference
 * side.
 *
 * Conventions
 *   - plain C types only; complex data is interleaved float (re, im), the
 *     layout of fftwf_complex / TYPECPX in the reference;
 *   - every function returns KG_OK (0) or a negative kg_status; nothing throws;
 *     kg_last_error() gives the text of the last failure on this thread;
 *   - "_dev" variants take pointers to device (HBM) memory and only enqueue
 *     work on the context's stream; the others take host memory, copy, and
 *     (where they return results) synchronise;
 *   - the library owns all device memory it allocates; callers keep ownership
 *     of every buffer they pass in;
 *   - footprint of a "_dev" call: it reads only the stated extent of every input row and writes only the stated extent of every
 *     output row (a row with count 0, a disabled channel, an output a mode does not produce: nothing); the bytes between a row's
 *     extent and its stride, in front of row 0 and behind the last row are neither read nor written, no input is written unless
 *     the call is told to work in place, and no output depends on what its buffer held before.  Each entry point states the
 *     alignment its pointers and strides need; a pointer that misses it is refused with KG_ERR_INVALID and nothing is enqueued
 *     (tests/test_containment_*_gpu.py hold every entry point to this, at exactly that alignment);
 *   - there is NO CPU fallback: without a usable gfx950 device kg_ctx_create
 *     fails with KG_ERR_NO_DEVICE.
 *   - the reference runs this path from cooperative coroutines on one host
 *     thread (support/coroutines.cpp); the async entry points plus kg_ctx_poll()
 *     are meant to be called around its NextTask() yield points.
 */
#ifndef KIWIGPU_H
#define KIWIGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KG_ABI_VERSION 4     /* 4 (round 6): kg_post_cfir_* / _squelch_* / _set_deemp (AM, NBFM reach d_s16), kg_rxbank_join / _leave /
                              * _audio_map / _ready, kg_fir_process_each_dev; 3 (round 5): kg_rxbank_*, kg_ddc_wf_step_dev; 2 (round 4): kg_wf_frames_at_dev takes the extent of d_iq; kg_ctx_mark */

typedef enum {
    KG_OK = 0,
    KG_ERR_NO_DEVICE = -1,   /* no HIP device / not gfx950 / HIP runtime failure at init */
    KG_ERR_INVALID = -2,     /* bad argument */
    KG_ERR_HIP = -3,         /* a HIP call failed; see kg_last_error() */
    KG_ERR_NOMEM = -4,
    KG_ERR_STATE = -5        /* call out of order (e.g. correlate before a code was set) */
} kg_status;

const char *kg_strerror(int status);
const char *kg_last_error(void);
int kg_abi_version(void);

/* Memory and failure.  A kg_*_create that fails leaves *out NULL and holds nothing: whatever it had allocated is released
 * before it returns.  An allocation the device refuses is KG_ERR_NOMEM, with the byte count and the buffer's name in
 * kg_last_error(), from every entry point; other HIP failures stay KG_ERR_HIP.  A call refused with KG_ERR_NOMEM leaves its
 * object as it was or with its grow-on-demand staging empty: the object stays usable, and the same call made again simply grows
 * the staging again.
 * kg_dev_live_allocs: the device and pinned host allocations the library holds in this process at this moment, kg_dev_alloc's
 * included (a leak check: the count is back at its earlier value once everything created since was destroyed). */
int64_t kg_dev_live_allocs(void);

/* ------------------------------------------------------------------------ */
/* Context: one per GPU per process.                                         */
/* ------------------------------------------------------------------------ */
typedef struct kg_ctx kg_ctx;

/* stream: a hipStream_t to enqueue on (e.g. the caller's or PyTorch's current
 * stream), or NULL to let the library create its own non-blocking stream. */
int kg_ctx_create(int device, void *stream, kg_ctx **out);
/* The same, but `stream` is always taken as given: NULL here means HIP's legacy default
 * ("null") stream, which is what torch.cuda.current_stream().cuda_stream is (0) when no
 * other stream was selected.  The library never destroys a caller's stream. */
int kg_ctx_create_on_stream(int device, void *stream, kg_ctx **out);
void kg_ctx_destroy(kg_ctx *ctx);
int kg_ctx_sync(kg_ctx *ctx);                 /* hipStreamSynchronize */
int kg_ctx_poll(kg_ctx *ctx);                 /* 1 = stream idle, 0 = busy, <0 error */
void *kg_ctx_stream(kg_ctx *ctx);             /* the hipStream_t in use */
int kg_ctx_device_name(kg_ctx *ctx, char *buf, size_t len);
int kg_ctx_num_cus(kg_ctx *ctx);

/* Device-memory helpers for callers that do not bring their own HIP runtime
 * (the reference's host is plain C++): allocate / free HBM, blocking copies on
 * the context's stream. */
int kg_dev_alloc(kg_ctx *ctx, size_t bytes, void **out);
int kg_dev_free(kg_ctx *ctx, void *ptr);
int kg_dev_upload(kg_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int kg_dev_download(kg_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
/* hipMemGetInfo of the context's device (lifecycle tests, capacity planning). */
int kg_dev_mem_info(kg_ctx *ctx, size_t *free_bytes, size_t *total_bytes);

/* HIP-event stopwatch on the context's stream (bench.py and C++ callers). */
int kg_timer_start(kg_ctx *ctx);
int kg_timer_stop(kg_ctx *ctx, float *elapsed_ms);    /* synchronises on the stop event */
/* Profiling aid: enqueues an empty kernel (`kg_mark_kernel`) of `tag` workgroups of 64 threads on the
 * context's stream (1 <= tag <= 65535).  Counter rows of `rocprofv3 --pmc`, which carry no timestamps
 * or user markers, can then be attributed to the phase between two tags by dispatch order
 * (bench.py's live HBM-traffic passes). */
int kg_ctx_mark(kg_ctx *ctx, int tag);

/* ------------------------------------------------------------------------ */
/* GPS C/A + E1B parallel-code-phase acquisition.                            */
/* Replaces gps/search.cpp: SearchInit() code tables (:183-350), Sample()    */
/* (:382-449), Correlate() (:453-499).                                       */
/* The reference's shape (gps/gps.h:62-73): NSAMPLES 65536, DECIM 4,          */
/* FFT_LEN 16384 -- what kg_acq_create() builds.  kg_acq_create_shape() builds */
/* the same algorithm for a longer coherent interval (BASELINE.json           */
/* configs[4]); every size below then reads kg_acq_nsamples() / kg_acq_fft_len() */
/* in place of the two constants.                                             */
/* ------------------------------------------------------------------------ */
#define KG_ACQ_NSAMPLES 65536
#define KG_ACQ_FFT_LEN  16384
#define KG_ACQ_DECIM    4         /* gps/gps.h:62 */
/* BASELINE.json configs[4]: 10 ms coherent at FS = 16.368 MHz, zero-padded to a
 * 65536-point transform at SAMPLE_RATE = FS/DECIM = 4.092 MHz.  One Doppler bin is
 * SAMPLE_RATE / FFT_LEN = 62.44 Hz there (249.76 Hz in the reference shape). */
#define KG_ACQ10_NSAMPLES 163680
#define KG_ACQ10_FFT_LEN  65536
#define KG_ACQ_L1_LIMIT 4092      /* SAMPLE_RATE/1000*L1_CODE_PERIOD,  search.cpp:486 */
#define KG_ACQ_E1B_LIMIT 16368    /* SAMPLE_RATE/1000*E1B_CODE_PERIOD, search.cpp:486 */

typedef struct kg_acq kg_acq;

/* Result of Correlate() for one SV.  valid == 0 means no Doppler bin had
 * snr > 0 (all-zero or NaN input): the reference then leaves its out-pointers
 * untouched and returns 0 (search.cpp:455,495). */
typedef struct { float snr; int32_t dop; int32_t idx; int32_t valid; } kg_acq_result;

/* One (SV, Doppler) cell of the search.cpp:465-496 loop. */
typedef struct { float snr; float max_pwr; float tot_pwr; int32_t idx; } kg_acq_cell;

/* max_sats: size of the code table (reference MAX_SATS = 64, gps.h:123).
 * dop_lo..dop_hi: Doppler bins searched (reference -20..20, search.cpp:465).
 * max_blocks: how many independent 65536-sample blocks ("receivers") can be
 * resident and searched in one launch. */
int kg_acq_create(kg_ctx *ctx, int max_sats, int dop_lo, int dop_hi, int max_blocks,
                  kg_acq **out);
/* The same engine for another shape of the same algorithm: a sample block holds
 * `nsamples` input samples at FS (a multiple of 8, at most DECIM * fft_len; the rest of
 * the DECIM * fft_len array Sample() decimates is zero, as DecimateBy2float's tail is,
 * search.cpp:145), the transforms are fft_len points (16384 or 65536), the code replica
 * covers all DECIM * fft_len samples as the reference's covers NSAMPLES (:250), a Doppler
 * bin is one bin of that transform, the peak-search windows stay 4092 / 16368.
 * kg_acq_create() == kg_acq_create_shape(.., KG_ACQ_NSAMPLES, KG_ACQ_FFT_LEN, ..). */
int kg_acq_create_shape(kg_ctx *ctx, int max_sats, int dop_lo, int dop_hi, int max_blocks,
                        int nsamples, int fft_len, kg_acq **out);
int kg_acq_nsamples(kg_acq *acq);
int kg_acq_fft_len(kg_acq *acq);
void kg_acq_destroy(kg_acq *acq);

/* SearchInit() per-SV body, run on the device: resample chips {0,1} at 16
 * samples/chip over NSAMPLES, Bipolar, (boc: XOR BOC(1,1), search.cpp:317),
 * 2x DecimateBy2float, forward FFT.  limit = peak-search window
 * (KG_ACQ_L1_LIMIT / KG_ACQ_E1B_LIMIT). */
int kg_acq_set_code(kg_acq *acq, int sat, const uint8_t *chips, int nchips, int boc,
                    int limit);
/* Upload a ready-made code spectrum (FFT_LEN complex, natural bin order), i.e.
 * the first half of the reference's code[sat][] (search.cpp:54,283). */
int kg_acq_set_code_fft(kg_acq *acq, int sat, const float *code_fft, int limit);
int kg_acq_get_code_fft(kg_acq *acq, int sat, float *code_fft);      /* natural order */

/* Sample(): packed 1-bit IF (8192 bytes, LSB first; verilog/gps/sampler.v) ->
 * data spectrum of block `block`. */
int kg_acq_sample_bits(kg_acq *acq, int block, const uint8_t *packed);
int kg_acq_sample_bits_dev(kg_acq *acq, int block, const void *d_packed);
/* Extension (BASELINE.json configs[1]): NSAMPLES complex int16 samples
 * (i,q interleaved) at the FS/4 IF; mix by (-j)^n, then as Sample().
 * _dev forms read nsamples / 8 bytes at d_packed (any address) resp. 4 * nsamples bytes per block at d_iq (d_iq and stride_bytes
 * multiples of 4) and write no caller memory. */
int kg_acq_sample_iq16(kg_acq *acq, int block, const int16_t *iq);
int kg_acq_sample_iq16_dev(kg_acq *acq, int block, const void *d_iq);
/* nblocks consecutive blocks from one device array, block b at d_iq + b*stride_bytes:
 * one launch set for all of them. */
int kg_acq_sample_iq16_batch_dev(kg_acq *acq, int first_block, int nblocks, const void *d_iq,
                                 size_t stride_bytes);
/* The same for nblocks blocks in host memory, stride_samples complex samples apart: copied
 * into the library's pinned staging region before the call returns, one transfer and one
 * front-end launch for the batch. */
int kg_acq_sample_iq16_batch(kg_acq *acq, int first, int nblocks, const int16_t *iq, size_t stride_samples);
/* Inject / read back Correlate()'s `data` argument (fwd_buf after Sample()),
 * FFT_LEN complex in natural bin order. */
int kg_acq_set_data_fft(kg_acq *acq, int block, const float *data_fft);
int kg_acq_get_data_fft(kg_acq *acq, int block, float *data_fft);
/* The FFT_LEN decimated time-domain samples Sample() feeds its FFT. */
int kg_acq_get_data_td(kg_acq *acq, int block, float *td);

/* Correlate() for nsats SVs x (dop_hi-dop_lo+1) bins x nblocks blocks
 * (blocks 0..nblocks-1), one launch.  Enqueue only: no stream synchronisation in steady
 * state, also when the SV list differs from the previous call's (the reference's
 * SearchTask loop asks for one SV at a time); the pair table goes through the context's
 * staging ring, whose slot reuse can wait on an event once 32 uploads are outstanding.
 * With fewer than 8 (block, SV) pairs in a launch -- that calling pattern -- the cells,
 * not the pairs, are dealt over the 8 XCDs, so one SV's bins use the whole GPU.
 * Stream model: Sample() and Correlate() run in order on the context's stream
 * (a second stream for Sample() is an opt-in experiment). */
int kg_acq_correlate_async(kg_acq *acq, int nblocks, const int *sats, int nsats);
int kg_acq_correlate_blocks_async(kg_acq *acq, int first_block, int nblocks, const int *sats,
                                  int nsats);
/* Wait and copy out.  results[nblocks*nsats] (block-major), cells may be NULL
 * or [nblocks*nsats*ndop]. */
int kg_acq_fetch(kg_acq *acq, kg_acq_result *results, kg_acq_cell *cells);
/* Convenience: async + fetch for one block. */
int kg_acq_correlate(kg_acq *acq, int block_count, const int *sats, int nsats,
                     kg_acq_result *results, kg_acq_cell *cells);
/* Device pointer to the last launch's kg_acq_result array (for RCCL gathers). */
void *kg_acq_results_dev(kg_acq *acq);

/* ------------------------------------------------------------------------ */
/* Waterfall frames.  Replaces, per (channel, frame): the unpack + window of   */
/* sample_wf() (rx/rx_waterfall.cpp:1049-1066) and compute_frame()             */
/* (:1275-1575: 8192-point FFT, power, CIC compensation, FFT-bin -> pixel      */
/* reduce, dB, clamp, u8).  The tables and maps stay the caller's: they are    */
/* the arrays c2s_waterfall_init() (:122-203) and the c2s_waterfall() loop     */
/* (:775-928) already build, passed as they are.                               */
/* ------------------------------------------------------------------------ */
#define KG_WF_NFFT  8192      /* WF_C_NFFT = WF_C_NSAMPS, rx/rx_waterfall.h:61-62 */
#define KG_WF_WIDTH 1024      /* WF_WIDTH, rx/rx_waterfall.h:65 */

typedef struct kg_wf kg_wf;

/* The scalar members of wf_inst_t (rx/rx_waterfall.h:118-157) compute_frame() reads. */
typedef struct {
    int32_t zoom;                 /* wf->zoom */
    int32_t window_func;          /* WINF_WF_* 0..3, rx_waterfall.h:160-163 */
    int32_t interp;               /* wf_interp_t: 0 MAX, 1 MIN, 2 LAST, 3 DROP, 4 CMA (rx_waterfall.h:116) */
    int32_t cic_comp;             /* wf->cic_comp */
    int32_t overlapped;           /* wf->overlapped_sampling */
    int32_t fft_used;             /* 4096 at zoom 0, 2048 otherwise (:756-763) */
    int32_t plot_width;           /* :772 */
    int32_t plot_width_clamped;   /* :773 */
    float fft_offset;             /* :898 */
} kg_wf_chan_cfg;

int kg_wf_create(kg_ctx *ctx, int nchan, kg_wf **out);
void kg_wf_destroy(kg_wf *wf);
/* wf_shmem_t.window_function[4][8192] and .CIC_comp[8192] (rx_waterfall.h:166-172) */
int kg_wf_set_tables(kg_wf *wf, const float *window_function, const float *cic_comp);
/* wf_inst_t.fft2wf_map[fft_used], .drop_sample[1024], .fft_scale[1024],
 * .fft_scale_div2[1024] of channel ch.  Only the "FFT >= plot" case (:1400) is
 * supported (fft_used >= plot_width), the only one reachable for FlyDog. */
int kg_wf_set_channel(kg_wf *wf, int ch, const kg_wf_chan_cfg *cfg, const uint16_t *fft2wf_map,
                      const uint16_t *drop_sample, const float *fft_scale,
                      const float *fft_scale_div2);
/* nframes frames; frame f belongs to channel chan_of[f] (host array), its input is
 * iq[f][8192] {int16 i, int16 q} (struct iq_t, :95-97) and its output out[f][1024]
 * bytes (wf_pkt_t.un.buf).  _dev: device pointers, enqueue only.  A frame's start is
 * kept as a 32-bit sample offset: nframes <= 524288 (2^32 / 8192) per call.
 * Alignment (all three _dev forms): d_iq 8 bytes (with even frame_off every frame then is), d_out 4 bytes (kg_wf_nb_frames_dev: 8).
 * Read: the 8192 pairs of each listed frame, nothing between or around frames; written: 1024 bytes per frame at d_out + 1024 f. */
int kg_wf_frames_dev(kg_wf *wf, int nframes, const int32_t *chan_of, const void *d_iq, void *d_out);
int kg_wf_frames(kg_wf *wf, int nframes, const int32_t *chan_of, const int16_t *iq, uint8_t *out);
/* The same for frames that are NOT back to back: frame f starts frame_off[f] samples (iq_t pairs; even,
 * below 2^32) after d_iq -- frames taken where the DDC left them (kg_ddc_wf_push_dev's per-channel rows),
 * the way sample_wf() reads the FPGA's sample ring in place (rx/rx_waterfall.cpp:1036-1066).  iq_len = how
 * many iq_t pairs d_iq points at: every frame must satisfy frame_off[f] + 8192 <= iq_len (KG_ERR_INVALID
 * otherwise -- an offset is never turned into a device read outside the caller's buffer). */
int kg_wf_frames_at_dev(kg_wf *wf, int nframes, const int32_t *chan_of, const uint64_t *frame_off,
                        uint64_t iq_len, const void *d_iq, void *d_out);
/* One frame with the intermediate arrays of compute_frame(): pwr[4096] (entries
 * below fft_used are written), pwr_out[1024], dB[1024] (before the clamp). */
int kg_wf_debug_frame(kg_wf *wf, int ch, const int16_t *iq, uint8_t *out, float *pwr,
                      float *pwr_out, float *dB);

/* The waterfall's noise blanker (rx/rx_waterfall.cpp:1087-1099, rx/CuteSDR/noiseproc.cpp): one CNoiseProc per channel, the
 * m_NoiseProc_wf[] array.  kg_wf_nb_setup is SetupBlanker("WF", 8192, nb_param) -- the sample rate is WF_C_NSAMPS, not the
 * channel's -- with kg_nb_setup's refusals; it resets the blanker in stream order.  kg_wf_set_nb switches the blanker of a
 * channel on or off (on: refused with KG_ERR_STATE for a channel that was never set up).  While it is on, every frame of that
 * channel in kg_wf_frames_dev / kg_wf_frames_at_dev / kg_wf_frames / kg_wf_debug_frame (which applies it as a one-frame call does)
 * is windowed and then run through ProcessBlankerOneShot(8192) -- its state carried from frame to frame in list order, the delay of
 * D + 1 with D samples skipped (the frame moves by one sample, its first sample is the previous frame's last), the zero flush --
 * before the transform.  A call without a blanked channel launches what it launched before. */
int kg_wf_nb_setup(kg_wf *wf, int ch, const float *nb_param /* [KG_NB_PARAMS] */);
int kg_wf_set_nb(kg_wf *wf, int ch, int on);
/* The standalone call site: window + ProcessBlankerOneShot for a list of frames (chan_of / frame_off / iq_len as
 * kg_wf_frames_at_dev; every listed channel set up, on or not), frame f written to d_out + f * 8192 as complex floats. */
int kg_wf_nb_frames_dev(kg_wf *wf, int nframes, const int32_t *chan_of, const uint64_t *frame_off, uint64_t iq_len,
                        const void *d_iq, void *d_out);
/* kg_nb_state's layout for the waterfall blankers.  Synchronises. */
int kg_wf_nb_state(kg_wf *wf, const int32_t *chans, int nch, int32_t *ints, float *flts);

/* ------------------------------------------------------------------------ */
/* Waterfall DDC.  In the reference this is FPGA fabric behind SPI commands:   */
/* WATERFALL_1CIC (verilog/rx/waterfall_1cic.v:20-144) = IQ_MIXER (iq_mixer.v)  */
/* + cic_prune_var "wf1" (cic_prune_var.v, cic_wf1.vh) + IQ_SAMPLER_8K_32B,     */
/* programmed with CmdSetWFFreq / CmdSetWFDecim / CmdWFReset and read with      */
/* CmdGetWFSamples (rx/rx_waterfall.cpp:466,507,1005,1036).  Here the ADC        */
/* stream is an int16 array in HBM and every listed channel is computed from it. */
/* ------------------------------------------------------------------------ */
typedef struct kg_ddc kg_ddc;

int kg_ddc_create(kg_ctx *ctx, int nchan, size_t max_samples, kg_ddc **out);
void kg_ddc_destroy(kg_ddc *ddc);
/* CmdSetWFFreq (48-bit phase increment, i_offset of rx_waterfall.cpp:498-507) and
 * CmdSetWFDecim (R = 1, 2, 4 .. 8192).  Also resets the channel (phase = 0). */
int kg_ddc_set_wf(kg_ddc *ddc, int ch, uint64_t phase_inc, int decim);
/* CmdWFReset with WF_SAMP_WR_RST: zero the CIC registers and the decimation
 * counter; the NCO phase keeps running. */
int kg_ddc_reset_wf(kg_ddc *ddc, int ch);
int kg_ddc_set_phase(kg_ddc *ddc, int ch, uint64_t phase);
/* The NCO sine / cosine tables both DDCs use (8192 int16 entries each, addressed by phase bits 47:35):
 * round(16383 cos / sin(2 pi a / 8192)) -- the frozen stand-in for the closed Xilinx DDS core of
 * verilog/rx/iq_mixer.v:60-65 (no dither).  Host function, needs no GPU; the device keeps the two as one
 * 10240-entry sine table (cos a = T[a + 2048]). */
int kg_ddc_nco_table(int16_t *cos_tab, int16_t *sin_tab);
/* IQ pairs channel ch will produce for the next n ADC samples. */
long kg_ddc_wf_outputs(kg_ddc *ddc, int ch, size_t n);
/* Run n ADC samples (device int16 array) through the listed channels.  Channel
 * chan_list[i] writes its IQ pairs {int16 i, int16 q} (struct iq_t) to
 * d_out + i*out_stride (in pairs); nouts[i] (may be NULL) receives the count.
 * State (NCO phase, CIC registers, decimation phase) carries over to the next
 * call, so a stream may be pushed in pieces of any length.  Enqueue only.
 * d_adc and the rows may sit at any 2- / 4-byte alignment (d_adc a multiple of 2, d_out of 4, any out_stride); R = 1 channels are
 * fastest (16-byte stores) when d_adc is 8-byte aligned and every row 16-byte aligned, i.e. d_out 16-byte aligned and out_stride
 * a multiple of 4.  Read: n samples at d_adc; written: the nouts[i] pairs of row i and nothing else, at either alignment (a 16-byte
 * store never runs past the last pair).  The same holds for kg_ddc_wf_capture_dev (min(max_out, n >> log2 R) pairs per row) and
 * kg_ddc_wf_step_dev (pairs out_off[i] .. out_off[i] + nouts[i] of row i: the pairs in front of out_off[i] are not written either). */
int kg_ddc_wf_push_dev(kg_ddc *ddc, const void *d_adc, size_t n, const int32_t *chan_list,
                       int nlist, void *d_out, size_t out_stride, int64_t *nouts);
/* The reference's NON-OVERLAPPED waterfall frame (sample_wf(), rx/rx_waterfall.cpp:1005-1041): CmdWFReset with
 * WF_SAMP_RD_RST | WF_SAMP_WR_RST -- verilog/rx/waterfall_1cic.v:45-47,106-128: both CICs (registers, decimation
 * counter) and the sampler's write pointer are cleared, the NCO keeps running -- then the ONE-SHOT sampler
 * (IQ_SAMPLER_8K_32B, wr_continuous = 0) fills with the next 8192 outputs and stops.  Here: the reset falls on the
 * block's first sample; channel chan_list[i] writes its first min(max_out, n >> log2 R) pairs to d_out + i*out_stride
 * and only the max_out * R samples that produce them reach its filters (a zoom-1 channel reads 8192 samples of a
 * 4 Mi-sample block, not all of it); every NCO advances by the whole block.  A channel captured from is left with its
 * filters stopped short: the next kg_ddc_wf_push_dev on it starts from the reset state, as the reference does when it
 * switches the sampler to continuous mode (CmdWFReset with WF_SAMP_CONTIN, :971-978).  Enqueue only. */
int kg_ddc_wf_capture_dev(kg_ddc *ddc, const void *d_adc, size_t n, const int32_t *chan_list,
                          int nlist, void *d_out, size_t out_stride, size_t max_out, int64_t *nouts);
/* Both sampler modes in ONE call (round 5; a bank of receivers, kg_rxbank below): entry i is pushed through the continuous
 * sampler when max_out[i] == 0 (as kg_ddc_wf_push_dev) and captured -- CmdWFReset at the block's first sample, then the
 * one-shot sampler of max_out[i] pairs -- when max_out[i] >= 1 (as kg_ddc_wf_capture_dev); its pairs go to
 * d_out + i*out_stride + out_off[i] (out_off may be NULL: all zero; out_off[i] + the entry's outputs <= out_stride), e.g. the
 * write position of a sample ring.  Enqueue only. */
int kg_ddc_wf_step_dev(kg_ddc *ddc, const void *d_adc, size_t n, const int32_t *chan_list, int nlist, void *d_out,
                       size_t out_stride, const int64_t *out_off, const int64_t *max_out, int64_t *nouts);
/* Deferred output stage (round 4) -- the non-blocking submit / poll form SURVEY 8(b) asks of the DDC seam (today every
 * CmdGetWFSamples is a blocking SPI transaction, platform/common/spi.cpp:487-507).  Off (default): everything a push
 * enqueues is ordered on the context's stream.  On: the push returns with its output stage (R = 1 bypass channels,
 * run-total prefix, combs: everything that WRITES d_out) on a stream of the object, and the context's stream carries
 * only the run passes -- the next push's run passes start while this push's outputs are still being written.
 *   kg_ddc_wf_join(ddc, stream)      `stream` (a hipStream_t; NULL: the context's) waits for the last push's outputs:
 *                                    call it on whichever stream reads d_out first.
 *   kg_ddc_wf_tail_after(ddc, event) the NEXT push's writers of d_out start only after `event` (a hipEvent_t the
 *                                    caller recorded behind its last reader of the rows): the write-after-read edge of
 *                                    a caller that still reads push k's rows while push k + 1 runs.  One-shot.
 * d_adc: whatever reads the caller's samples is ordered on the context's stream before the push returns (in both modes), so
 * the caller may refill or recycle d_adc on that stream right behind the push; only the rows need kg_ddc_wf_join.
 * Every other entry point of the object drains the deferred work first. */
int kg_ddc_wf_set_deferred(kg_ddc *ddc, int on);
int kg_ddc_wf_join(kg_ddc *ddc, void *stream);
int kg_ddc_wf_tail_after(kg_ddc *ddc, void *event);

/* ------------------------------------------------------------------------ */
/* Audio DDC.  In the reference: one RX instance per audio channel in FPGA      */
/* fabric (verilog/rx/rx.v:22-178): IQ_MIXER (22 bits) -> CIC N=3 R=1736 ->      */
/* CIC N=5 R=3 -> 65-tap CICF /2 (fir_iq.sv) -> 24-bit IQ at ADC/10416 (the rx4 / */
/* rx8 instance; rx3 and rx14: kg_rxddc_create_mode), read as                     */
/* rx_iq_t records with CmdGetRX (rx/data_pump.cpp:101) after the NCO was set    */
/* with CmdSetRXFreq (rx/rx_sound_cmd.cpp:41-51).                                */
/* ------------------------------------------------------------------------ */
typedef struct kg_rxddc kg_rxddc;

int kg_rxddc_create(kg_ctx *ctx, int nchan, size_t max_samples, kg_rxddc **out);   /* KG_RXDDC_STD */
/* The RX instances the reference builds, selected by its RX_CFG (kiwi.config:101-105, 140-143;
 * verilog/rx/fir_iq.sv:39-123; register widths as verilog/rx/cic_gen.c emits them):
 *   KG_RXDDC_STD   rx4 / rx8: CIC 1736 -> CIC 3 -> 65-tap CICF / 2 = ADC / 10416 (12 kHz class)
 *   KG_RXDDC_WIDE  rx3:       CIC 1543 -> CIC 2 -> 65-tap CICF (RX_CFG == 3 taps) / 2 = ADC / 6172 (20.25 kHz)
 *   KG_RXDDC_RX14  rx14:      CIC 1736 -> CIC 3 -> 17-tap CICF (RX_CFG == 14 taps) / 2 = ADC / 10416 */
enum { KG_RXDDC_STD = 0, KG_RXDDC_WIDE = 1, KG_RXDDC_RX14 = 2 };
int kg_rxddc_create_mode(kg_ctx *ctx, int nchan, size_t max_samples, int mode, kg_rxddc **out);
int kg_rxddc_decim(kg_rxddc *ddc);                          /* ADC samples per output record */
void kg_rxddc_destroy(kg_rxddc *ddc);
/* CmdSetRXFreq: 48-bit phase increment i_phase = round(f / adc_clk * 2^48).  The
 * filters keep running across a retune, as in the FPGA. */
int kg_rxddc_set_freq(kg_rxddc *ddc, int ch, uint64_t phase_inc);
int kg_rxddc_reset(kg_rxddc *ddc, int ch);                 /* power-on state */
long kg_rxddc_outputs(kg_rxddc *ddc, int ch, size_t n);     /* records the next n samples yield */
/* n ADC samples (device int16 array) through the listed channels: channel
 * chan_list[i] writes nouts[i] rx_iq_t records {u16 i, u16 q, u8 q3, u8 i3}
 * (rx/data_pump.h:27-30) to d_out + i*out_stride records.  State carries over
 * between calls.  Enqueue only.  d_adc and d_out: multiples of 2 bytes (a record is 6 bytes: rows are 2-byte aligned at any
 * out_stride).  Read: n samples at d_adc and nothing behind them (16 bytes at a time where a run of the stream starts at a
 * 16-byte address, sample by sample elsewhere).  Written: 6 * nouts[i] bytes of row i. */
int kg_rxddc_push_dev(kg_rxddc *ddc, const void *d_adc, size_t n, const int32_t *chan_list,
                      int nlist, void *d_out, size_t out_stride, int32_t *nouts);

/* ------------------------------------------------------------------------ */
/* Audio front: data-pump unpack and the CFastFIR passband filter.             */
/* ------------------------------------------------------------------------ */
/* snd_service() unpack (rx/data_pump.cpp:145-208): nsamps * nchans rx_iq_t records
 * {u16 i, u16 q, u8 q3, u8 i3} (rx/data_pump.h:27-30), sample-major / channel-minor,
 * -> out[ch][nsamps] TYPECPX: re = q*rescale + DC_offset_I, im = i*rescale +
 * DC_offset_Q (I and Q as given when spectral_inversion).  enabled[ch] == 0 leaves
 * that channel's output untouched (rx_channels[ch].data_enabled).  Device buffers;
 * enabled is a host array.  Synchronous.  d_raw: a multiple of 2 bytes, d_out of 8 (out_stride in complex samples; both unpack
 * calls).  Read: the 6 * nsamps bytes of each record row (here: 6 * nsamps * nchans bytes); written: 8 * nsamps bytes of every
 * enabled channel's row. */
int kg_dpump_unpack_dev(kg_ctx *ctx, const void *d_raw, int nsamps, int nchans,
                        const uint8_t *enabled, float rescale, float dc_i, float dc_q,
                        int spectral_inversion, void *d_out, size_t out_stride);

/* The same unpack for records stored one row per channel, raw_stride records apart: the
 * layout kg_rxddc_push_dev writes (many receivers, no SPI interleave).  Enqueue only. */
int kg_dpump_unpack_rows_dev(kg_ctx *ctx, const void *d_raw, size_t raw_stride, int nsamps, int nchans,
                             const uint8_t *enabled, float rescale, float dc_i, float dc_q,
                             int spectral_inversion, void *d_out, size_t out_stride);

#define KG_FIR_FFT_SIZE 1024      /* CONV_FFT_SIZE, rx/CuteSDR/cuteSDR.h:12 */
#define KG_FIR_OUT      512       /* FASTFIR_OUTBUF_SIZE, rx/CuteSDR/cuteSDR.h:14 */

typedef struct kg_fir kg_fir;      /* the m_PassbandFIR[MAX_RX_CHANS] array, rx/rx_sound.cpp:150 */

/* max_in: the largest InLength of one ProcessData call. */
int kg_fir_create(kg_ctx *ctx, int nchan, int max_in, kg_fir **out);
void kg_fir_destroy(kg_fir *fir);
/* CFastFIR::SetupParameters(instance, FLoCut, FHiCut, Offset, SampleRate)
 * (rx/CuteSDR/fastfir.cpp:171-232) with the window of SetupWindowFunction
 * (:102-146; window_func < 0 = Blackman-Nuttall) and SetupCICFilter (:148-158;
 * snd_rate_3ch selects the :70-71 constants).  Taps are designed on the host in
 * the reference's float arithmetic, transformed on the device.  Returns 1 when the
 * sanity check (:193-200) rejects the parameters and the old filter stays. */
int kg_fir_setup(kg_fir *fir, int ch, float FLoCut, float FHiCut, float Offset, float SampleRate,
                 int window_func, int do_cic_comp, int snd_rate_3ch);
/* Or hand over the reference's own m_pFilterCoef_CIC[1024] (complex float); the channel's m_CIC[] is
 * then 1.0 (m_do_CIC_comp false, what FlyDog builds: fastfir.cpp:94). */
int kg_fir_set_coef(kg_fir *fir, int ch, const float *coef_fft);
int kg_fir_get_coef(kg_fir *fir, int ch, float *coef_fft);
int kg_fir_reset(kg_fir *fir, int ch);
int kg_fir_pos(kg_fir *fir, int ch);                        /* CFastFIR::FirPos(), fastfir.h:33 */
/* CFastFIR::ProcessData(rx_chan, InLength, In, Out) (fastfir.cpp:241-324), host
 * buffers: returns the number of complex samples written to out (0 or a multiple
 * of 512), or a negative status. */
int kg_fir_process(kg_fir *fir, int ch, const float *in, int n, float *out);
/* The same for a list of channels at once, device buffers: channel chans[i] takes
 * n samples from d_in + i*in_stride and writes nout[i] samples to d_out + i*out_stride
 * (strides in complex samples).  Enqueue only.  Every device buffer of the kg_fir_*_dev calls (d_in, d_out, d_pre, d_post) is read
 * and written as complex floats: 8-byte aligned, else KG_ERR_INVALID.  Read: n (n_each[i]) samples of row i; written: 8 * nout[i]
 * bytes of row i, nothing for a row that completes no block. */
int kg_fir_process_dev(kg_fir *fir, const int32_t *chans, int nch, const void *d_in,
                       size_t in_stride, int n, void *d_out, size_t out_stride, int32_t *nout);
/* The same with an InLength of its own for every listed channel (n_each[i] >= 0 samples at row i of d_in): connections whose
 * audio DDCs were started at different times deliver different record counts in one data-pump interval. */
int kg_fir_process_each_dev(kg_fir *fir, const int32_t *chans, int nch, const void *d_in, size_t in_stride,
                            const int32_t *n_each, void *d_out, size_t out_stride, int32_t *nout);

/* ---------------------------------------------------------------------------
 * The standard noise blanker, NB_STD (rx/CuteSDR/noiseproc.cpp, CNoiseProc): the m_NoiseProc_snd[] array of rx/rx_sound.cpp.
 * Its audio call site (rx_sound.cpp:593-598, NB_STD_POST_FILTER undefined) runs ProcessBlanker in place on the unpacked block,
 * right before CFastFIR, when nb_enable[NB_BLANKER] && nb_algo == NB_STD. */
enum { KG_NB_OFF = 0, KG_NB_STD = 1, KG_NB_WILD = 2 };                           /* nb_algo_e, rx/rx_noise.h:6 */
enum { KG_NB_BLANKER = 0, KG_NB_WF = 1, KG_NB_CLICK = 2 };                       /* nb_type_e, rx/rx_noise.h:7 */
enum { KG_NB_GATE = 0, KG_NB_THRESHOLD = 1,                                      /* extensions/noise_blank/noise_blank.h */
       KG_NB_PARAMS = 8 };                                                       /* NOISE_PARAMS, rx/rx_noise.h:4 */
#define KG_NB_MAG_CAP 1024         /* the largest m_MagSamples (0.005 x sample rate) a setup accepts */

typedef struct kg_nb kg_nb;

/* max_in: the largest InLength of one ProcessBlanker call. */
int kg_nb_create(kg_ctx *ctx, int nchan, int max_in, kg_nb **out);
void kg_nb_destroy(kg_nb *nb);
/* SetupBlanker(id, sample_rate, nb_param) (noiseproc.cpp:89-145), in stream order: m_GateSamples = (int) (GateUsec * 1e-6 *
 * SampleRate) clamped to [3, 4096], m_MagSamples = (int) (0.005 * SampleRate) at least 1, the threshold clamped to [0, 100] (NaN
 * passes), m_Ratio = .005 * Threshold * M, m_DelaySamples = G / 2; pointers, counter, sum and both rings reset.  sample_rate 0:
 * only the reset.  Refused (nothing changes): KG_ERR_INVALID for a gate product that is NaN or outside int, a sample rate that is
 * NaN, infinite or gives m_MagSamples above KG_NB_MAG_CAP; KG_ERR_STATE for sample rate 0 on a channel never set up. */
int kg_nb_setup(kg_nb *nb, int ch, float sample_rate, const float *nb_param /* [KG_NB_PARAMS] */);
/* ProcessBlanker(n_each[i], in, out) (noiseproc.cpp:147-203) on complex floats (TYPECPX) for each listed channel: n_each[i] >= 0
 * samples from row i of d_in to row i of d_out (rows chans[i] on a receiver bank's context, kg_ctx::rows_by_chan; strides in
 * complex samples; d_in == d_out allowed).  A channel that was never set up is refused with KG_ERR_STATE (the reference's rings
 * are uninitialised there).  Nothing is launched when every count is 0.  Enqueue only.  d_in and d_out: 8-byte aligned; in place
 * needs in_stride == out_stride.  Read and written: 8 * n_each[i] bytes of row i. */
int kg_nb_process_dev(kg_nb *nb, const int32_t *chans, int nch, const void *d_in, size_t in_stride, const int32_t *n_each,
                      void *d_out, size_t out_stride);
/* The same for one channel with host buffers; synchronous (in == out allowed). */
int kg_nb_process(kg_nb *nb, int ch, const float *in, int n, float *out);
/* The state of each listed channel: ints[6 i ..] = m_Mptr, m_Dptr, m_BlankCounter, m_MagSamples, m_DelaySamples, m_GateSamples;
 * flts[2 i ..] = m_Ratio, m_MagAveSum (either may be NULL).  Synchronises. */
int kg_nb_state(kg_nb *nb, const int32_t *chans, int nch, int32_t *ints, float *flts);

/* ---------------------------------------------------------------------------
 * What consumes the CFastFIR output in c2s_sound(), per receiver channel
 * (SURVEY.md 8(f) rank 1): S-meter (rx/rx_sound.cpp:248-250, 676-696), the m_Agc[]
 * array (rx/rx_sound.cpp:152; rx/CuteSDR/agc.cpp) and the AM / NBFM detectors
 * (rx/rx_sound.cpp:766-783, 845-881).  One object holds these for nchan receivers;
 * kg_post_process_dev() runs a batch of channels in one launch (one wavefront per
 * channel: the recursions are sequential per channel, parallel across channels).
 * ------------------------------------------------------------------------- */
typedef struct kg_post kg_post;

enum {                      /* what follows the S-meter for a channel (the `switch (s->mode)` of :763-900) */
    KG_POST_IQ   = 0,       /* MODE_IQ/DRM: CAgc complex -> complex (rx_sound.cpp:1096-1100)                      -> d_agc */
    KG_POST_SSB  = 1,       /* MODE_USB/USN/LSB/LSN/CW/CWN: CAgc complex -> mono16 (:893)                         -> d_s16 */
    KG_POST_AM   = 2,       /* MODE_AM/AMN: CAgc, envelope, DC-removal IIR (:766-783) -> d_demod; m_AM_FIR (:787) -> d_s16 */
    KG_POST_NBFM = 3,       /* MODE_NBFM/NNFM: CAgc, fmdemod_quadri + clipper (:845-875) -> d_demod;
                             * m_Squelch.PerformFMSquelch (:876, rx/CuteSDR/squelch.cpp:151-231)                  -> d_s16 */
    /* the synchronous-AM family (:791-806): CAgc, then wdsp_SAM_demod() (rx/wdsp/SAM_demod.cpp:210-356) over the AGC output */
    KG_POST_SAM  = 4,       /* MODE_SAM: corr[I]; with a channel null (kg_post_set_sam_mparam) the nulled sideband   -> d_s16
                             * (and (audion, 0) / (0, audion) written over d_agc, as over agc_samps_c)                 */
    KG_POST_SAU  = 5,       /* MODE_SAU: the upper sideband of the phase-shifted products                           -> d_s16 */
    KG_POST_SAL  = 6,       /* MODE_SAL: the lower sideband                                                          -> d_s16 */
    KG_POST_SAS  = 7,       /* MODE_SAS: (lsb, usb) over d_agc; stereo (IS_STEREO): no d_s16, the packet is IQ payload    */
    KG_POST_QAM  = 8        /* MODE_QAM: C-QUAM (L, R) = corr[I] +- corr[Q] over d_agc; stereo as SAS                     */
};                          /* SSB, AM, NBFM, SAM, SAU, SAL: then the de-emphasis filter over d_s16 in place when it is on
                             * (:898-907; the SAM family takes the AM / SSB filter)                                       */

#define KG_POST_MAX_SAMPLES 1024  /* per call and channel; c2s_sound() hands over ns_out = 512 */

int kg_post_create(kg_ctx *ctx, int nchan, kg_post **out);
void kg_post_destroy(kg_post *post);
/* CAgc::SetParameters(AgcOn, UseHang, Threshold, ManualGain, SlopeFactor, Decay, SampleRate)
 * (agc.cpp:98-163): returns at once when nothing changed; a new sample rate clears the
 * delay line, the magnitude window and the averagers.  Constants are computed on the
 * host with the reference's float/double expressions.  A fresh object is in the state
 * the reference reaches after its first call with a new sample rate. */
int kg_post_set_agc(kg_post *post, int chan, int agc_on, int use_hang, int threshold, int manual_gain,
                    int slope_factor, int decay, float sample_rate);
int kg_post_agc_delay(kg_post *post, int chan);           /* CAgc::GetDelaySamples(), agc.h:27 */
/* sMeterAlpha = 1 - expf(-1 / (frate * ATTACK_TIMECONST)) (rx_sound.cpp:248-249) */
int kg_post_set_smeter(kg_post *post, int chan, float frate);
int kg_post_set_mode(kg_post *post, int chan, int mode);
int kg_post_get_mode(kg_post *post, int chan);              /* -> KG_POST_*, or < 0 */
/* The three libm functions the device code of this path calls, over an array: y[i] = f(x[i]), or, with d_x NULL, f of the float
 * whose bit pattern is first_bits + i.  KG_MATH_LOG10F: the S-meter's and CAgc's log10f (rx/rx_sound.cpp:687, rx/CuteSDR/agc.cpp:191;
 * CAgc BRANCHES on it, :215-240); KG_MATH_POWF: powf(base, x), CAgc's gain with base 10 (agc.cpp:250-253; base positive, finite,
 * normal); KG_MATH_EXPF: aperture_auto()'s IIR gain (rx/rx_waterfall.cpp:1199).  The reference calls the platform's libm; the device
 * functions restate the GNU C Library 2.35 algorithms of this image (csrc/kg_libm.h) and equal them bit for bit on every argument
 * (tests/test_libm_gpu.py, tools/check_libm.py --exhaustive), which is what makes the audio chain's outputs the reference's own bits.
 * Enqueue only.  d_x, d_y (and kg_math_atan2f_dev's three arrays): 4-byte aligned; 4 * n bytes read resp. written. */
enum { KG_MATH_LOG10F = 0, KG_MATH_POWF = 1, KG_MATH_EXPF = 2,
       KG_MATH_SINF = 3, KG_MATH_COSF = 4 };   /* the SAM PLL's sinf / cosf of its phase error (rx/wdsp/SAM_demod.cpp:218-219) */
int kg_math_dev(kg_ctx *ctx, int fn, float base, const void *d_x, uint32_t first_bits, size_t n, void *d_y);
/* d_out[i] = atan2f(d_y[i], d_x[i]): the SAM PLL's phase detector (SAM_demod.cpp:331), the image's glibc 2.35 e_atan2f.c restated
 * (csrc/kg_libm_trig.h; tests/test_sam_libm_gpu.py, tools/check_sam_libm.cpp).  Enqueue only. */
int kg_math_atan2f_dev(kg_ctx *ctx, const void *d_y, const void *d_x, size_t n, void *d_out);
/* A new connection on the channel: sMeterAvg_dB = 0, z1 = 0 (rx_sound.cpp:244,250),
 * conn->last_sample = 0, wdsp_SAM_PLL(PLL_MED) + wdsp_SAM_PLL(PLL_RESET) (:302-303).  The AGC object persists across
 * connections, as m_Agc[] does. */
int kg_post_reset(kg_post *post, int chan);
/* The synchronous-AM demodulator of a channel (rx/wdsp/SAM_demod.cpp).  kg_post_set_mode from a non-SAM mode into KG_POST_SAM ..
 * KG_POST_QAM resets its PLL, and every mode change clears isChanNull (rx_sound_cmd.cpp:214-226).
 * kg_post_sam_setup: wdsp_SAM_demod_init() (:154-163) for the server's nominal snd_rate, 12000 or 20250 (not frate): omega_min / max
 * and the fade leveler's constants; the PLL gains are recomputed at that rate.  A fresh object is at 12000, PLL MED, reset.
 * kg_post_sam_pll: wdsp_SAM_PLL(type) (:113-152), `SET sam_pll=%d` (rx_sound_cmd.cpp:444-451): -1 PLL_RESET (the previous type,
 * state cleared), 0 DX, 1 MED, 2 FAST.  kg_post_set_sam_mparam: s->SAM_mparam = mparam & MODE_FLAGS_SAM (rx_sound_cmd.cpp:216):
 * bits 0-1 the channel null (1 LSB, 2 USB), 4 FADE_LEVELER, 8 DC_BLOCK (wdsp.h:5-10).  The gains and constants are computed on the
 * host with the reference's float / double expressions and the host libm. */
int kg_post_sam_setup(kg_post *post, int chan, int snd_rate);
int kg_post_sam_pll(kg_post *post, int chan, int type);
int kg_post_set_sam_mparam(kg_post *post, int chan, int mparam);
/* After the last pass: carrier[i] = wdsp_SAM_carrier() (SAM_demod.cpp:165-170, the UI's carrier offset in Hz, NaN -> 0),
 * is_chan_null[i] = s->isChanNull (rx_sound.cpp:802), phzerror[i] = the PLL's phase.  Any output may be NULL.  Synchronises. */
int kg_post_sam_state(kg_post *post, const int32_t *chans, int nch, float *carrier, int32_t *is_chan_null, float *phzerror);
/* One pass over nsamps FIR output samples of each listed channel (d_fir + i*in_stride,
 * complex float).  Outputs (any may be NULL) at row i*out_stride of d_s16 (int16: out_samps_s2, every
 * mode but IQ, SAS and QAM), d_demod (float: the detector's output, AM / NBFM), d_agc (complex float: the AGC's output,
 * every mode but SSB; in SAS / QAM the stereo pair and in channel-null SAM the nulled pair written over it, rx_sound.cpp:802).  Float -> mono16 is
 * the reference's (TYPEMONO16) cast: truncation; outside the int16 range (undefined in
 * C) the low 16 bits of the int32 conversion, as x86 does.  Enqueue only.
 * Alignment: d_fir and d_agc 8 bytes, d_demod 4, d_s16 2 (each dereferenced as its element type; in_stride / out_stride in
 * elements, ONE out_stride for the three outputs), else KG_ERR_INVALID.  Read: nsamps samples of row i of d_fir.  Written: nsamps
 * elements of row i of each output the channel's mode produces; a row of an output the mode does NOT produce is not written at
 * all -- d_s16 in IQ / SAS / QAM, d_demod in every mode but AM / NBFM, d_agc in SSB -- and keeps what the caller left there. */
int kg_post_process_dev(kg_post *post, const int32_t *chans, int nch, const void *d_fir, size_t in_stride,
                        int nsamps, void *d_s16, void *d_demod, void *d_agc, size_t out_stride);
/* The noise-reduction switch of c2s_sound() (rx/rx_sound.cpp:933-949), after the de-emphasis filter and the NBFM squelch, in place
 * on out_samps_s2 of every mode but the stereo ones (KG_POST_IQ, KG_POST_SAS, KG_POST_QAM): the auto-notch first, then the denoiser,
 * each when enabled.  The two LMS algorithms: NR_WDSP, wdsp's variable-leak LMS (rx/wdsp/ANR.cpp), and NR_ORIG,
 * the 121-tap LMS (rx/kiwi/lms.cpp), bit for bit (the third, NR_SPECTRAL, has calls of its own below: kg_post_nrs_*).  kg_post_process_dev runs it over its d_s16 rows for every listed channel whose
 * algo is KG_NR_WDSP or KG_NR_ORIG with a type enabled; such a batch needs d_s16 (NULL is refused with KG_ERR_INVALID: the
 * filter states must advance as the reference's do).  A batch with no such channel launches what it launched before. */
enum { KG_NR_OFF = 0, KG_NR_WDSP = 1, KG_NR_ORIG = 2, KG_NR_SPECTRAL = 3 };     /* nr_algo_e, rx/rx_noise.h:9 */
enum { KG_NR_DENOISE = 0, KG_NR_AUTONOTCH = 1 };                                 /* nr_type_e, rx/rx_noise.h:10 */
enum { KG_NR_DELAY = 0, KG_NR_BETA = 1, KG_NR_DECAY = 2,                         /* NR_ORIG's parameters, extensions/noise_filter/noise_filter.h */
       KG_NR_TAPS = 0, KG_NR_DLY = 1, KG_NR_GAIN = 2, KG_NR_LEAKAGE = 3,         /* NR_WDSP's */
       KG_NR_PARAMS = 8 };                                                       /* NOISE_PARAMS, rx/rx_noise.h:4 */
/* The three commands, with the reference's side effects.
 * kg_post_set_nr_algo: `SET nr algo=` (rx_sound_cmd.cpp:464-471): the algo, and both enables cleared; no filter state changes.
 * kg_post_set_nr_enable: `SET nr type= en=` (:505-510): any nonzero en enables.
 * kg_post_set_nr_param: `SET nr type= param= pval=` (:511-521): the value is stored, then type `type` of the CURRENT algo is
 * initialised from the whole stored vector of that type (wdsp_ANR_init or CLMS::Initialize, on the host in the reference's types);
 * under any other algo only the value is stored.
 * The filter objects of each algo and type persist across algo switches, mode changes (kg_post_set_mode leaves NR alone) and
 * connections; kg_post_reset clears the algo (KG_NR_OFF), the enables and the stored parameters, as a new connection does
 * (rx_sound.cpp:236-240).  A fresh object's filters are zeroed, as the reference's statics start: an enabled filter that was never
 * initialised runs as that zero state does (a never-initialised CLMS is a denoiser in either slot).
 * Refused with KG_ERR_INVALID, the inputs on which the reference is undefined or which are not implemented:
 *   KG_NR_SPECTRAL in kg_post_set_nr_algo (it is selected by kg_post_nrs_select, which carries its passband rule);
 *   a type other than KG_NR_DENOISE / KG_NR_AUTONOTCH (m_LMS[ch][2] is out of bounds);
 *   a param index outside 0..7;
 *   under KG_NR_WDSP, a vector whose taps or delay is NaN, infinite or outside int (the (int) conversion), taps > 512 (overruns
 *   w[]) or delay > INT_MAX - 1022 (in_idx + j + delay overflows); under KG_NR_ORIG, a NaN delay-line length (its conversion).
 *   The value is then not stored. */
int kg_post_set_nr_algo(kg_post *post, int chan, int algo);
int kg_post_set_nr_enable(kg_post *post, int chan, int type, int en);
int kg_post_set_nr_param(kg_post *post, int chan, int type, int param, float pval);
/* The standalone call site: wdsp_ANR_filter(ch, type, ...) or m_LMS[ch][type].ProcessFilter(...) under each listed channel's current
 * algo (KG_NR_WDSP or KG_NR_ORIG, else KG_ERR_STATE), whatever its enables and mode: nsamps int16 at row i of d_in -> row i of d_out
 * (d_in == d_out allowed).  The same device code as the fused pass.  Enqueue only.  The three standalone stages (this one,
 * kg_post_nrs_process_dev, kg_post_nbw_process_dev): d_in and d_out 2-byte aligned, strides in int16 elements; read and written:
 * 2 * nsamps bytes of row i. */
int kg_post_nr_process_dev(kg_post *post, const int32_t *chans, int nch, int type, const void *d_in, size_t in_stride, int nsamps,
                           void *d_out, size_t out_stride);
/* The filter states of `type` for the listed channels, any output may be NULL: anr_i[3 i ..] = wdsp in_idx, taps, delay;
 * anr_f[2 i ..] = lidx, ngamma; lms_i[3 i ..] = CLMS m_dlp, m_dlen, m_nr_type; anr_w[512 i ..] = wdsp w[]; lms_coef[121 i ..] =
 * m_lmscoef[].  Synchronises. */
int kg_post_nr_state(kg_post *post, const int32_t *chans, int nch, int type, int32_t *anr_i, float *anr_f, int32_t *lms_i,
                     float *anr_w, float *lms_coef);
/* NR_SPECTRAL, the third algorithm of that switch (rx/rx_sound.cpp:945-947 -> rx/Teensy/NR_spectral.cpp, the UHSDR spectral-weighting
 * denoiser): per 512 samples two 50 %-overlapped 512-point frames, each windowed, transformed (CMSIS arm_cfft_f32, radix 8), weighted
 * per passband bin and transformed back; the output lags the input by 256 samples.  Bit for bit against the reference's code run with
 * the transform tables of DESIGN.md ("Spectral noise reduction": the reference tree declares them and defines them nowhere).  It runs
 * whenever the algo is KG_NR_SPECTRAL and the mode is not a stereo one; the enables are not consulted (:945-947).  One state per
 * channel (nr_spectral[], NR_spectral.cpp:69), kept across algo switches, modes and connections like the LMS states; a state that
 * was never initialised is all zeros and runs as such (final_gain 0: silence), as in the reference.
 * kg_post_nrs_select: `SET nr algo=3` (rx_sound_cmd.cpp:464-471): algo = KG_NR_SPECTRAL, both enables cleared, no state touched.  Any
 *   kg_post_set_nr_algo afterwards leaves it; kg_post_reset returns to KG_NR_OFF, zeroes the passband (memset(s)) and keeps the state.
 * kg_post_set_nr_param under KG_NR_SPECTRAL (:520): stores the value and runs nr_spectral_init from that type's whole stored vector
 *   (KG_NRS_GAIN, KG_NRS_ALPHA, KG_NRS_ASNR; either type index re-parameterises the one state); the first one per channel also
 *   arms the start-up phase (first_time = 1) and seeds four arrays (NR_spectral.cpp:85-101).
 * kg_post_nrs_setup: the reference's global snd_rate as this stage sees it: tinc .. ap (NR_spectral.cpp:89-93, host libm) and the bin
 *   width of the passband.  One value per object (the reference's are file-scope); 12000 until called.
 * kg_post_nrs_passband: s->norm_locut / norm_hicut as rx_sound_cmd.cpp:252-266 forms them from the clamped cuts of `SET mod=
 *   low_cut= high_cut=` (:248-250); VAD_low / VAD_high follow (NR_spectral.cpp:214-238).  kg_post_set_am_passband is unchanged.
 * The passband rule: NR_spectral.cpp's smoothing loops (:284-314) index NR_G[] down to VAD_high - 2 NN + 1 and up to VAD_low + NN/2
 *   + NN - 2 with a data-dependent NN <= 9, i.e. outside the arrays unless VAD_high >= 17 and VAD_low <= 244 (at 12 kHz: a
 *   norm_hicut above about 375 Hz).  The command that would put a KG_NR_SPECTRAL channel on such a passband is refused with
 *   KG_ERR_INVALID and the previous setting kept: kg_post_nrs_select, kg_post_nrs_passband, kg_post_nrs_setup.
 * kg_post_process_dev runs the stage over its d_s16 rows for every listed channel with KG_NR_SPECTRAL in a mono mode; such a batch
 *   needs d_s16 and nsamps % 512 == 0 (KG_ERR_INVALID, nothing enqueued).  A batch without such a channel launches what it launched before. */
enum { KG_NRS_MAX_SAMPLES = 4096 };                              /* kg_post_nrs_process_dev: at most eight blocks a call */
enum { KG_NRS_GAIN = 0, KG_NRS_ALPHA = 1, KG_NRS_ASNR = 2 };      /* NR_S_GAIN, NR_ALPHA, NR_ASNR, extensions/noise_filter/noise_filter.h:24-26 */
int kg_post_nrs_select(kg_post *post, int chan);
int kg_post_nrs_setup(kg_post *post, int snd_rate);
int kg_post_nrs_passband(kg_post *post, int chan, double locut, double hicut);
/* The standalone call site: nr_spectral_process(ch, 512, ...) once per 512 samples of row i of d_in -> row i of d_out (d_in == d_out
 * allowed) for each listed channel (its algo must be KG_NR_SPECTRAL, else KG_ERR_STATE), whatever its mode.  nsamps: a positive
 * multiple of 512 (the reference asserts 512) up to KG_NRS_MAX_SAMPLES, else KG_ERR_INVALID.  The same device code as the fused pass.  Enqueue only. */
int kg_post_nrs_process_dev(kg_post *post, const int32_t *chans, int nch, const void *d_in, size_t in_stride, int nsamps, void *d_out,
                            size_t out_stride);
/* The states of the listed channels, any output may be NULL: ints[4 i ..] = first_time, init_counter, VAD_low, VAD_high;
 * scalars[8 i ..] = final_gain, alpha, asnr, xih1, xih1r, pfac, norm_locut, norm_hicut; rate[6] = tinc, tax, tap, ax, ap, snr_prio_min;
 * arrays[9 * 256 i ..] = last_sample_buffer, last_iFFT_result, NR_Nest, xt, pslp, NR_SNR_post, NR_SNR_prio, NR_Hk_old, NR_G.  Synchronises. */
int kg_post_nrs_state(kg_post *post, const int32_t *chans, int nch, int32_t *ints, float *scalars, float *rate, float *arrays);
/* NB_WILD, the second algorithm of the noise-blanker switch (rx/rx_sound.cpp:922-931 -> rx/Teensy/NB_Wild.cpp, Michael Wild's LPC
 * blanker): per 512 samples an LPC model of the block (order = taps), the block inverse- and matched-filtered, up to 20 impulses found
 * above thresh * sqrt(variance * coefficient power), and impulse_samples | 1 samples around each replaced by the cross-fade of a forward
 * and a backward prediction.  The output is the input delayed by order + PL samples (PL = ((impulse_samples | 1) - 1) / 2) with the
 * repaired stretches; every output sample equals the reference's.  It sits behind de-emphasis and ahead of the noise-reduction switch,
 * in the modes that are not stereo ones.  One state per channel (nb_Wild[], NB_Wild.cpp:36), kept across modes and connections.
 * kg_post_nbw_init: nb_Wild_init (NB_Wild.cpp:38-46; called by `SET nb type=0 param= pval=` under NB_WILD, rx_sound_cmd.cpp:498):
 *   zeroes the whole state, the history included, then takes thresh, (s1_t) taps and (s1_t) impulse_samples from nb_param[KG_NBW_THRESH,
 *   KG_NBW_TAPS, KG_NBW_SAMPLES] (a value outside signed char, whose conversion C leaves undefined, is recorded as 0).  A vector is
 *   usable when thresh is finite, taps is 1..40 and impulse_samples 2..41: with taps 0 or fewer than 2 samples the reference divides 0
 *   by 0 and NaN samples reach its output, beyond 40 / 41 it leaves its arrays.  Storing is never refused while the stage is off (the
 *   client's three parameter messages pass through unusable vectors); with the stage on an unusable vector is KG_ERR_INVALID, nothing changed.
 * kg_post_set_nbw: the stage's switch, s->nb_enable[NB_BLANKER] && s->nb_algo == NB_WILD (rx_sound.cpp:924-929), held by the caller.
 *   Switching on with an unusable vector is KG_ERR_STATE.  kg_post_reset clears the switch and keeps the state, as memset(s) does.
 * kg_post_process_dev runs the stage behind post_kernel and ahead of the NR stages over its d_s16 rows for every listed channel with the
 *   switch on in a mono mode; such a batch needs d_s16 and nsamps % 512 == 0 (KG_ERR_INVALID, nothing enqueued).  A batch without such
 *   a channel launches what it launched before. */
enum { KG_NBW_MAX_SAMPLES = 4096 };                              /* kg_post_nbw_process_dev: at most eight blocks a call */
enum { KG_NBW_THRESH = 0, KG_NBW_TAPS = 1, KG_NBW_SAMPLES = 2 };  /* NB_THRESH, NB_TAPS, NB_SAMPLES, extensions/noise_blank/noise_blank.h */
enum { KG_NBW_HIST = 120 };                                      /* 2 * 40 + 2 * 20: the most a call carries to the next */
int kg_post_nbw_init(kg_post *post, int chan, const float *nb_param /* [KG_NB_PARAMS] */);
int kg_post_set_nbw(kg_post *post, int chan, int on);
/* The standalone call site: nb_Wild_process(ch, 512, ...) (NB_Wild.cpp:253-261) once per 512 samples of row i of d_in -> row i of d_out
 * (d_in == d_out allowed) for each listed channel, whatever its mode and switch; its vector must be usable, else KG_ERR_STATE.  nsamps:
 * a positive multiple of 512 up to KG_NBW_MAX_SAMPLES, else KG_ERR_INVALID.  The same device code as the fused pass.  Enqueue only. */
int kg_post_nbw_process_dev(kg_post *post, const int32_t *chans, int nch, const void *d_in, size_t in_stride, int nsamps, void *d_out,
                            size_t out_stride);
/* The states of the listed channels, either output may be NULL: ints[3 i ..] = taps, impulse_samples, the switch; floats[121 i ..] =
 * thresh, then working_buffer[0 .. KG_NBW_HIST) of which a call writes the first 2 * order + 2 * PL (the rest is 0).  Synchronises. */
int kg_post_nbw_state(kg_post *post, const int32_t *chans, int nch, int32_t *ints, float *floats);
/* The CFir objects of a channel (rx/rx_sound.cpp:153-156; rx/CuteSDR/fir.cpp): the filter behind the AM detector and the
 * two de-emphasis filters.  (CSquelch owns a fourth, its noise high-pass: kg_post_squelch_setup.) */
enum { KG_CFIR_AM = 0, KG_CFIR_DEEMP_NFM = 1, KG_CFIR_DEEMP_AM_SSB = 2,
       KG_CFIR_SQUELCH_HP = 3 };     /* CSquelch::m_HpFir: readable and runnable, designed only by kg_post_squelch_setup */
enum { KG_CFIR_REAL_REAL = 0, KG_CFIR_REAL_MONO16 = 1, KG_CFIR_MONO16_MONO16 = 2 };   /* the ProcessFilter overloads, fir.cpp:74, :176, :199 */
/* CFir::InitLPFilter(NumTaps, Scale, Astop, Fpass, Fstop, Fsamprate) (fir.cpp:282-384): Kaiser-windowed sinc designed on the
 * host in the reference's float arithmetic; clears the filter's sample buffer.  Returns the tap count (9..97), or < 0. */
int kg_post_cfir_init_lp(kg_post *post, int chan, int which, int NumTaps, float Scale, float Astop, float Fpass,
                         float Fstop, float Fsamprate);
/* CFir::InitConstFir(NumTaps, pCoef, Fsamprate) (fir.cpp:220-240): the caller's coefficients (the reference hands over a row
 * of rx/rx_filter.h's de-emphasis tables, rx/rx_sound_cmd.cpp:556-585); more than 97 are cut to 97.  Returns the tap count. */
int kg_post_cfir_init_const(kg_post *post, int chan, int which, int NumTaps, const float *coef, float Fsamprate);
int kg_post_cfir_get_taps(kg_post *post, int chan, int which, float *taps);    /* -> tap count; taps may be NULL */
/* m_*_FIR[chan].ProcessFilter(nsamps, in, out) on its own, for a list of channels (rows in_stride / out_stride elements apart;
 * float or int16 by `kind`; in == out allowed): the same device code as inside kg_post_process_dev.  The sums run in the
 * reference's order (fir.cpp:79-91: over the circular buffer's positions, so the first tap of the sum rotates with the
 * write position): bit-exact.  Enqueue only.  Float rows 4-byte aligned, int16 rows 2-byte (by `kind`, in and out each), else
 * KG_ERR_INVALID; nsamps elements of row i read and written. */
int kg_post_cfir_process_dev(kg_post *post, const int32_t *chans, int nch, int which, int kind, const void *d_in, size_t in_stride,
                             int nsamps, void *d_out, size_t out_stride);
/* m_Squelch[chan].PerformFMSquelch(nsamps, in, out) on its own (squelch.cpp:151-231): float detector samples -> mono16 (1 when
 * squelched); the return values through kg_post_squelch_state.  Enqueue only.  d_in 4-byte aligned (4 * nsamps bytes of row i
 * read), d_out 2-byte (2 * nsamps bytes written). */
int kg_post_squelch_perform_dev(kg_post *post, const int32_t *chans, int nch, const void *d_in, size_t in_stride, int nsamps,
                                void *d_out, size_t out_stride);
/* The post-AM-detector filter as a passband change designs it (rx/rx_sound_cmd.cpp:248-250, 268-282): the cuts clamped to
 * +-(frate / 2 - 1) as the handler clamps s->locut / s->hicut (a no-op for a caller that passes those), hbw = max(|hicut|, |locut|)
 * capped at frate / 2, stop = 1.8 hbw capped at frate / 2, m_AM_FIR.InitLPFilter(0, 1.0, 50.0, hbw, stop, frate).  Returns the
 * tap count.  A channel in KG_POST_AM mode without it is refused (the reference's undesigned CFir holds garbage). */
int kg_post_set_am_passband(kg_post *post, int chan, double locut, double hicut, double frate);
/* "SET de_emp=%d nfm=%d" (rx/rx_sound_cmd.cpp:543-554): s->deemp_nfm (nfm != 0) or s->deemp = de_emp; non-zero turns the
 * corresponding filter on for the channel's NBFM resp. AM / SSB modes (do_de_emp, rx/rx_sound.cpp:482).  The coefficients
 * come through kg_post_cfir_init_const. */
int kg_post_set_deemp(kg_post *post, int chan, int nfm, int de_emp);
/* CSquelch (rx/CuteSDR/squelch.cpp) of a channel: SetupParameters(rx_chan, samplerate) (:84-116; designs the noise high-pass,
 * InitHPFilter(0, 1.0, 50.0, 2400, 1950, samplerate), and resets), SetSquelch(Value, SquelchMax) (:122-129; SquelchMax 0 =
 * 8192), Reset() (:67-77).  rx/rx_sound.cpp:261-262 calls the first two for every new connection; a channel in KG_POST_NBFM
 * mode without them is refused.  (The reference clears conn->last_sample with Reset(), rx/rx_sound_cmd.cpp:238-239: that
 * is kg_post_reset's.) */
int kg_post_squelch_setup(kg_post *post, int chan, float samplerate);
int kg_post_squelch_set(kg_post *post, int chan, int Value, int SquelchMax);
int kg_post_squelch_reset(kg_post *post, int chan);
/* After the last pass: nsq_nc_sq[i] = what PerformFMSquelch returned for channel chans[i] (-1 opened, 0 no change, +1 closed),
 * squelched[i] = s->squelched as rx/rx_sound.cpp:877 keeps it (SND_FLAG_SQUELCH_UI, :1232), ave[i] = m_SquelchAve.  Any
 * output may be NULL.  Synchronises the stream. */
int kg_post_squelch_state(kg_post *post, const int32_t *chans, int nch, int32_t *nsq_nc_sq, int32_t *squelched, float *ave);
/* S-meter state after the last pass: avg_dB[i] = sMeterAvg_dB, and (taps != NULL)
 * taps[2i], taps[2i+1] = the values receive_S_meter() is handed at j == 0 and j == ns_out/2
 * (rx_sound.cpp:693), all before S_meter_cal is added.  Synchronises the stream. */
int kg_post_smeter(kg_post *post, const int32_t *chans, int nch, float *avg_dB, float *taps);

/* ---------------------------------------------------------------------------
 * Wire formats: the IMA ADPCM coder of rx/csdr/ima_adpcm.cpp
 * as c2s_sound() and compute_frame() use it, the waterfall packet and the sound packet
 * header, so that what leaves the GPU is byte-compatible with the web client.
 * Integer work: bit-exact.
 * ------------------------------------------------------------------------- */
typedef struct kg_adpcm kg_adpcm;   /* the per-connection `ima_adpcm_state_t adpcm_snd` (rx/rx_sound.h) of nchan channels */

int kg_adpcm_create(kg_ctx *ctx, int nchan, kg_adpcm **out);
void kg_adpcm_destroy(kg_adpcm *a);
/* memset(&s->adpcm_snd, 0, ...) is set_state(chan, 0, 0); get_state() is what the
 * "MSG audio_adpcm_state=%d,%d" message carries (rx/rx_sound.cpp:1314): index, previousValue. */
int kg_adpcm_set_state(kg_adpcm *a, int chan, int index, int previous);
int kg_adpcm_get_state(kg_adpcm *a, int chan, int *index, int *previous);
/* encode_ima_adpcm_i16_e8(out_samps_s2, bp_real_u1, ns_out, &s->adpcm_snd) (ima_adpcm.cpp:185-197,
 * rx/rx_sound.cpp:1122) for a list of channels: row i of d_s16 (int16, in_stride samples apart)
 * -> nsamps/2 bytes at d_out + i*out_stride (bytes).  nsamps even.  Enqueue only.  d_s16: a multiple of 2 bytes; d_out and
 * out_stride: any. */
int kg_adpcm_encode_dev(kg_adpcm *a, const int32_t *chans, int nch, const void *d_s16, size_t in_stride,
                        int nsamps, void *d_out, size_t out_stride);
/* The uncompressed payload (rx/rx_sound.cpp:1126-1140): int16 rows copied as they are
 * (little_endian != 0) or byte-swapped to network order.  Enqueue only.  d_s16, d_out and out_stride (bytes): multiples of 2;
 * 2 * nsamps bytes of row i read and written. */
int kg_snd_payload_dev(kg_ctx *ctx, const void *d_s16, size_t in_stride, int nch, int nsamps,
                       int little_endian, void *d_out, size_t out_stride);
/* The IQ modes' payload (rx/rx_sound.cpp:1076-1096; MODE_IQ, and SAS / QAM / DRM monitor with their own sources): row i of d_cpx
 * (complex float: the AGC's output, d_agc of kg_post_process_dev) -> nsamps x {(s2_t) re, (s2_t) im}, 4 nsamps bytes at
 * d_out + i*out_stride, little-endian as they are or in network order.  chans: NULL (rows 0 .. nch-1), or the channel list
 * (a receiver bank's rows go by channel).  Enqueue only.  d_cpx: 8-byte aligned; d_out and out_stride (bytes): multiples of 2. */
int kg_snd_iq_payload_dev(kg_ctx *ctx, const int32_t *chans, int nch, const void *d_cpx, size_t in_stride, int nsamps,
                          int little_endian, void *d_out, size_t out_stride);
/* The 10 header bytes of snd_pkt_real_t (rx/rx_sound.h:42-48; rx/rx_sound.cpp:252,
 * 1219-1254): "SND", flags, seq little-endian, S-meter clamped to -127 .. 3.4 dBm and sent
 * big-endian in 0.1 dB steps above -127.  Host only. */
void kg_snd_header(uint8_t flags, uint32_t seq, float smeter_dBm, uint8_t *h);

/* The GPS time stamp of snd_pkt_iq_t (rx/rx_sound.h:61-64), host arithmetic as c2s_sound() does it.
 * State per sound connection (snd_t::gpssec, last_gpssec, gps_init, rx/rx_sound.h:120-122). */
typedef struct { double gpssec, last_gpssec; int32_t gps_init; int32_t pad; } kg_gps_state;
typedef struct { uint32_t gpssec, gpsnsec; uint8_t last_gps_solution; uint8_t pad[3]; } kg_iq_stamp;
/* rx/rx_sound.cpp:557, once per data-pump buffer: gpssec = fmod(week + clk.gps_secs + dticks /
 * clk.adc_clock_base - gps_delay + gps_delay2, week); dticks = the buffer's 48-bit tick count minus
 * clk.ticks. */
void kg_snd_gps_begin(kg_gps_state *s, double clk_gps_secs, double dticks, double adc_clock_base,
                      double gps_delay, double gps_delay2);
/* rx/rx_sound.cpp:636-661, once per 512-sample FIR output block: the FIR delay (norm_nrx_samps -
 * fir_pos, fir_pos = kg_fir_pos() before the block) and the AGC delay (kg_post_agc_delay(), when the
 * AGC is on) are taken off, the header carries the PREVIOUS block's time (last_gpssec), and
 * last_gps_solution = 255 without a clock solution (clk_ticks == 0), else min(252, seconds since it),
 * 0 on the first block of a connection. */
void kg_snd_gps_stamp(kg_gps_state *s, int norm_nrx_samps, int fir_pos, int agc_on, int agc_delay,
                      int rx_decim, double adc_clock_base, double clk_gps_secs, uint64_t clk_ticks,
                      kg_iq_stamp *out);

#define KG_WF_ADPCM_PAD 10                          /* ADPCM_PAD, rx/rx_waterfall.h:83 */
#define KG_WF_PKT_HDR   16                          /* id4, x_bin_server, flags_x_zoom_server, seq */
#define KG_WF_PKT_MAX   (KG_WF_PKT_HDR + KG_WF_ADPCM_PAD + 1024)   /* sizeof(wf_pkt_t) */
typedef struct {
    uint32_t x_bin_server;          /* wf->start or wf->prev_start (rx_waterfall.cpp:1603-1616) */
    uint32_t zoom;                  /* wf->zoom or wf->prev_zoom; WF_FLAGS_COMPRESSION is added here */
    uint32_t seq;                   /* wf->snd_seq (:1635) */
    int32_t use_compression;        /* wf->compression, the connection's setting; a row at zoom 0 is never compressed (:1283-1285) */
} kg_wf_pkt_info;
/* wf_pkt_t for nrows waterfall rows (1024 u8 each, row_stride bytes apart, as
 * kg_wf_frames_dev leaves them): header + either the row or, compressed, the 10 pad bytes
 * (copies of the first pixel) and the row through encode_ima_adpcm_u8_e8 with a fresh state
 * (rx_waterfall.cpp:1622-1631).  Packet i starts at d_pkts + i*pkt_stride (>= KG_WF_PKT_MAX);
 * pkt_bytes[i] (host) = what goes on the wire: 16 + wf->out_bytes.  Enqueue only.  Any alignment (bytes).  Read: 1024 bytes of
 * row i; written: exactly pkt_bytes[i] bytes of packet i -- the rest of a compressed packet's KG_WF_PKT_MAX is not touched. */
int kg_wf_packets_dev(kg_ctx *ctx, const void *d_rows, size_t row_stride, int nrows,
                      const kg_wf_pkt_info *info, void *d_pkts, size_t pkt_stride, int32_t *pkt_bytes);

/* ---------------------------------------------------------------------------
 * Hand-off: what turns the path's results into the reference's
 * own programming.
 * ------------------------------------------------------------------------- */
typedef struct {
    double lo_dop, ca_dop;          /* Hz: Doppler from the FFT bin shift, and of the code rate */
    uint32_t lo_rate, ca_rate;      /* CmdSetRateLO / CmdSetRateCG words */
    uint32_t ca_pause;              /* CmdPause takes ca_pause - 1 when ca_pause != 0 */
    int32_t code_creep;             /* samples */
} kg_chan_start;
/* The arithmetic of CHANNEL::Start(sat, t_sample, lo_shift, ca_shift, snr)
 * (gps/channel.cpp:281-311) for a kg_acq_result: lo_shift = result.dop, ca_shift =
 * result.idx * DECIM (gps/search.cpp:575), secs = (timer_us() - t_sample) / 1e6.
 * Host only, double arithmetic as in the reference. */
void kg_acq_chan_start(int is_e1b, int lo_shift, int ca_shift, double secs, kg_chan_start *out);

typedef struct kg_aper kg_aper;     /* wf_inst_t::avg_pwr[APER_PWR_LEN] of nchan waterfalls (rx/rx_waterfall.h:154) */
enum { KG_APER_IIR = 0, KG_APER_MMA = 1, KG_APER_EMA = 2 };      /* aper_algo_t, rx/rx_waterfall.h:113 */
typedef struct {
    int32_t algo;                   /* KG_APER_*; a single-shot request is MMA with param 8 (:1192-1195) */
    float param;                    /* wf->aper_param */
    int32_t clear;                  /* wf->avg_clear: load the averages from this row (:1183-1188) */
    int32_t audio_fft;              /* rx_chan >= wf_chans: pixels 256..767 only (:1180-1181) */
} kg_aper_cfg;
int kg_aper_create(kg_ctx *ctx, int nchan, kg_aper **out);
void kg_aper_destroy(kg_aper *a);
/* The averaging half of aperture_auto() (rx/rx_waterfall.cpp:1183-1222) for row i of d_rows
 * (1024 u8 pixels, row_stride apart) and channel chans[i]; pixels go through dB_wire_to_dBm()
 * with waterfall_cal (rx/rx_util.cpp:905-912).  Enqueue only.  Any alignment; 1024 bytes of row i are read, no caller memory is
 * written. */
int kg_aper_update_dev(kg_aper *a, const int32_t *chans, int nrows, const void *d_rows, size_t row_stride,
                       const kg_aper_cfg *cfg, int waterfall_cal);
/* The reporting half (:1233-1272): signal = highest 5 dB band present (at least -80), noise =
 * the most populated band (the lowest of equals); bands <= -190 are masked areas; no band
 * at all gives -110 / -120.  Averages must lie within -190 .. 1000 dBm.  Synchronises. */
int kg_aper_report(kg_aper *a, const int32_t *chans, int n, const int32_t *audio_fft, int32_t *signal,
                   int32_t *noise);
int kg_aper_get(kg_aper *a, int chan, float *avg_pwr);            /* 1024 floats */

/* ---------------------------------------------------------------------------
 * GPS tracking channels: what receives the words of kg_acq_chan_start.  A bank of up to KG_TRK_MAX_CHANS channels, each the DEMOD
 * of verilog/gps/demod.v (code NCO, C/A generator of cacode.v or the E1B code memory, E/P/L replicas, 1-bit mixers, six 20-bit
 * integrators) plus the soft CPU's per-epoch service of e_cpu/kiwi.gps.asm (GPS_Method: CloseLoop on ip*qp and on pe-pl, the
 * lock flag, the nav-bit machine), clock for clock, on the packed 1-bit stream kg_acq_sample_bits_dev takes (LSB first in bytes).
 * Everything is integer; the library is held equal to a literal clock-by-clock model (tools/trk_model.cpp).
 *
 * What the reference leaves open and this API fixes:
 *   - the service delay.  The firmware writes the new NCO words some clocks after ms0, how many depends on its polling and on the
 *     other channels.  Here: lo_delay and cg_delay clocks after the clock edge that sets ms0 (2 <= lo_delay <= cg_delay <= 8183;
 *     0 selects KG_TRK_LO_DELAY / KG_TRK_CG_DELAY, the count of the listing for a channel serviced alone).  A word written at edge
 *     e acts from edge e + 1 on.  lo_delay > cg_delay is refused: GPS_Method is ONE instruction stream in which
 *     wrReg SET_LO_NCO comes before the code loop's arithmetic starts, so the reference cannot write the code word first; and an
 *     epoch's record, appended when its service completes (the code word's write), carries the LO word that service wrote.  An ms0 that arrives while a service is still due replaces it (one srq, one service).
 *   - the E1B code memory's own pipeline: after every full_chip the latched code is the memory chip at the new nchip.
 *   - registers without a reset value start at 0, cg_en at 1, gps.v's pause counter at 0.
 * Host commands act between process calls.  A command or getter after a process call waits for the stream, and the first process
 * call after a command waits for the upload of the channels' state; calls with no command between them only enqueue.
 * ------------------------------------------------------------------------- */
typedef struct kg_trk kg_trk;
enum { KG_TRK_MAX_CHANS = 12,            /* GPS_MAX_CHANS */
       KG_TRK_E1B_MODE = 0x800, KG_TRK_G2_INIT = 0x400,    /* the CmdSetSat word: E1B_MODE | g2_init | init[10:1] */
       KG_TRK_E1B_CODELEN = 4092, KG_TRK_CHAN_BYTES = 78,  /* sizeof GPS_CHAN (kiwi.gps.asm:31-45) */
       KG_TRK_LO_DELAY = 216, KG_TRK_CG_DELAY = 577,
       KG_TRK_MIN_EPOCH = 8184,          /* clocks: 1023 chips at the largest accepted code rate */
       KG_TRK_UNLOCKED = 1, KG_TRK_INAV = 2 };             /* kg_trk_epoch.flags */
typedef struct {
    uint64_t clock;                 /* the clock edge (0 = the first the bank consumed) that saw ms1: ser_iq latched, the filters restarted */
    int32_t ip, qp, ie, qe, il, ql; /* the six 20-bit counts the firmware reads, sign-extended */
    uint32_t lo_rate, cg_rate;      /* the NCO words after this epoch's service (with the loop off: as set) */
    uint32_t flags;                 /* KG_TRK_UNLOCKED: ch_unlocked != 0; KG_TRK_INAV: ip[19] */
    uint32_t reserved;              /* 0 */
} kg_trk_epoch;
int kg_trk_create(kg_ctx *ctx, int nchan, int lo_delay, int cg_delay, kg_trk **out);
void kg_trk_destroy(kg_trk *trk);
/* CmdSetSat.  C/A with taps needs both taps in 1..10 (cacode.v indexes g2[T]); afterwards the channel does not run before a
 * kg_trk_sampler_reset reaches it (the generator is seeded by `rst` only). */
int kg_trk_set_sat(kg_trk *trk, int ch, int codegen_init);
int kg_trk_set_e1b_code(kg_trk *trk, int ch, const uint8_t *chips, int nchips);     /* nchips == 4092, chips 0 / 1 */
/* SetRate: the integrator <- rate << 32, the NCO word <- rate.  cg: 2^27 <= rate < 2^29 (8 .. 32 clocks per chip; nominal 2^28),
 * else KG_ERR_INVALID: the closed form relies on nested chip events at least two clocks apart. */
int kg_trk_set_rate_lo(kg_trk *trk, int ch, uint32_t rate);
int kg_trk_set_rate_cg(kg_trk *trk, int ch, uint32_t rate);
int kg_trk_set_gain_lo(kg_trk *trk, int ch, int ki, int kp_minus_ki);               /* each 0..63 */
int kg_trk_set_gain_cg(kg_trk *trk, int ch, int ki, int kp_minus_ki);
int kg_trk_set_polarity(kg_trk *trk, int ch, int polarity);                         /* 0..2 */
int kg_trk_set_mask(kg_trk *trk, uint32_t mask);                                    /* CmdSetMask: bit ch set = not reset */
int kg_trk_sampler_reset(kg_trk *trk);                                              /* CmdSample's rst on the unmasked channels */
/* SET_PAUSE: cg_en <- 0 on channel ch, the bank's ONE pause counter <- count (0..65535); the generator stands for count + 1
 * clocks (a second pause moves the first one's end, gps.v:190-200).
 * A paused channel's chip events are held.  Held with nchip 0 at a half chip they would hold ms0 set and restart the filters every
 * clock; that state is not computed.  The command that would lead to it -- this one, kg_trk_set_rate_cg on a paused channel, or a
 * kg_trk_sampler_reset that reaches a paused channel whose service is still due -- is refused with KG_ERR_STATE and changes
 * NOTHING: the bank runs on.  For a pause that is about 9 clocks of a 16368-clock epoch (the 8 clocks after an ms0, while nchip is
 * still 0 and the service is due, and the held half chip itself): process 16 clocks more and pause then, with the count reduced
 * by those clocks. */
int kg_trk_pause(kg_trk *trk, int ch, int count);
int kg_trk_set_loop(kg_trk *trk, int ch, int on);       /* ours, not the reference's: off = the service leaves integrators and NCO words alone */
/* nclocks >= 1 clocks of every channel.  d_bits: the byte holding the next bit; the bit offset inside it carries over from the
 * previous call ((clocks consumed so far) % 8), so a stream may be cut anywhere.  Read: ceil((offset + nclocks) / 8) bytes.  One
 * kg_trk_epoch per completed service is appended to row ch (d_epochs + ch * chan_stride, 8-byte aligned, chan_stride >= cap
 * records); d_counts[ch] (device, int32) = how many: exactly that many records are written.  cap >= nclocks / 8184 + 2, else
 * KG_ERR_INVALID.  Enqueue only (see above).  KG_ERR_INVALID, nothing done: a channel without kg_trk_set_sat, or not reset since, or in
 * E1B mode without a code, or without a code rate.
 * A channel whose own code loop writes a word outside [2^27, 2^29) STOPS at that clock (the closed form does not hold there): its
 * count comes back as -1 - n (n records written before the stop), in this and in every later call, kg_trk_get_chan answers
 * KG_ERR_STATE and, after any command, so does this call; kg_trk_set_rate_cg starts the channel again from where it stopped (the
 * clocks in between are lost to it).  The other channels are not affected. */
int kg_trk_process_bits_dev(kg_trk *trk, const uint8_t *d_bits, size_t nclocks, kg_trk_epoch *d_epochs, size_t chan_stride, int cap,
                            int32_t *d_counts);
int kg_trk_process_bits(kg_trk *trk, const uint8_t *bits, size_t nclocks, kg_trk_epoch *epochs, size_t chan_stride, int cap,
                        int32_t *counts);               /* the same on host memory; synchronises */
int kg_trk_get_chan(kg_trk *trk, int ch, uint8_t *out);                             /* KG_TRK_CHAN_BYTES bytes: GPS_CHAN as CmdGetChan uploads it */
int kg_trk_get_clocks(kg_trk *trk, uint64_t *clock, uint32_t *replicas);            /* clocks consumed; the 18-bit replica word of each channel */

/* ---------------------------------------------------------------------------
 * Nav frame sync: what CHANNEL::Tracking() does with the nav bits of a channel -- the `holding` loop (gps/channel.cpp:441-506),
 * CHANNEL::ParityCheck (:731-832), L1_parity (:125-135) and, for Galileo, E1B_subframe (gps/GNSS-SDRLIB/sdrnav_gal.cpp:382-514): the
 * 30 x 8 de-interleave, KA9Q's K = 7 rate-1/2 Viterbi decoder (gps/ka9q-fec/viterbi27_port.cpp, polynomials 0x4f / 0x6d, metrics
 * from 63 / 0 without renormalisation, ties keep m0, chainback past 6 decisions from state 0), the even/odd test, checkcrc_e1b
 * (:293-319, CRC-24Q), the alert bits and the health bits decode_word5 reads (:163-174).  All integer, equal to the reference bit for bit.
 *
 * A channel is C/A (frames of 300 bits) or E1B (pages of 500 symbols).  It holds the reference's buf / holding and the index of
 * buf[0] in the channel's stream.  Pushed bits are appended; then, while holding >= 300 / 500, the head is judged as ParityCheck
 * judges it and nbits are dropped: 1 without a preamble (C/A: 8 bits, either polarity; E1B: the 10 symbols at the head and again
 * 250 later, the same polarity); C/A 30 (i + 1) when word i is the first to fail L1_parity, 300 after ten good words; E1B 250 on
 * GPS_ERR_SLIP, else 500.  Every head that passes the preamble test gives one kg_nav_frame, in stream order.  No decision depends
 * on holding beyond holding >= 300 / 500, so the records do not depend on how the stream is cut into pushes.
 *
 * Not here: whatever reads a validated frame into doubles or statistics (Ephemeris[].Subframe, decode_word0..10 and with them
 * nav.tow_updated: kg_eph, below; CHANNEL::Subframe); probation, alert, abort, bits_tow and
 * expecting_preamble, which are host decisions on id, err, bit and the count of bits pushed (bits_tow = holding - subframe_bits
 * depends on the reference's 16-bit polling grain: `bit` replaces it); the gps_debug dropped-subframe simulation and TEST_VECTOR.
 * ------------------------------------------------------------------------- */
typedef struct kg_nav kg_nav;
enum { KG_NAV_L1 = 0, KG_NAV_E1B = 1,
       KG_NAV_ERR_SLIP = 1, KG_NAV_ERR_CRC = 2, KG_NAV_ERR_ALERT = 3, KG_NAV_ERR_OOS = 4, KG_NAV_ERR_PAGE = 5,   /* GPS_ERR_*, gps/gps.h:187-191 */
       KG_NAV_ERR_PARITY = 16,           /* C/A: L1_parity failed (the reference returns no code of its own, only nbits) */
       KG_NAV_MAX_PUSH = 65536,          /* bits (epochs) per channel and call */
       KG_NAV_MAX_HELD = 499 };
typedef struct {
    uint64_t bit;          /* index of the frame's first bit in the channel's stream (0 = the first bit pushed since kg_nav_set_mode) */
    int32_t  err;          /* 0; C/A: KG_NAV_ERR_PARITY; E1B: KG_NAV_ERR_SLIP .. KG_NAV_ERR_PAGE (PAGE cannot occur: a 6-bit id is 0..63) */
    int32_t  consumed;     /* the nbits ParityCheck returns */
    int32_t  inverted;     /* 0 / 1 */
    int32_t  id;           /* C/A: bits 49..51 of the corrected buffer, MSB first (the subframe number, as Ephemeris reads it); on a parity
                              error the index of the failing word.  E1B: the word type as E1B_subframe returns it (on a CRC error
                              getbitu(dec_e1b1, 2, 6); on SLIP and ALERT 0) */
    uint8_t  data[40];     /* C/A and err == 0: the 300 bits as buf holds them after L1_parity, MSB first, 38 bytes + 2 zero; E1B:
                              dec_e1b1[15] then dec_e1b2[15], then 10 zero; C/A parity error: all zero */
} kg_nav_frame;
int kg_nav_create(kg_ctx *ctx, int nchan, kg_nav **out);                            /* 1 <= nchan <= KG_TRK_MAX_CHANS; every channel C/A and empty */
void kg_nav_destroy(kg_nav *nav);
/* KG_NAV_L1 or KG_NAV_E1B; empties the channel, restarts its stream index and its nav-bit machine, as Tracking() does on entry (:399-407).
 * In stream order, without waiting. */
int kg_nav_set_mode(kg_nav *nav, int ch, int mode);
/* Appends nbits[ch] (host array, one per channel, 0 .. KG_NAV_MAX_PUSH) bits to every channel and runs the loop above.  d_bits + ch *
 * chan_stride: one byte per bit, of which only bit 0 is read, as buf is; exactly nbits[ch] bytes of row ch are read.  Records go to row
 * ch of d_frames (d_frames + ch * frame_stride, 8-byte aligned, frame_stride >= cap), d_counts[ch] (device, int32) = how many: exactly
 * that many records and nchan counts are written.  cap >= the largest of ceil(nbits[ch] / 30) over the C/A channels and ceil(nbits[ch]
 * / 250) over the E1B ones, else KG_ERR_INVALID with nothing done: a record's head lies at least 30 / 250 bits behind the one before it, and
 * with at most 299 / 499 bits held the heads of one call span nbits[ch] positions.  Enqueue only. */
int kg_nav_push_bits_dev(kg_nav *nav, const uint8_t *d_bits, size_t chan_stride, const int32_t *nbits, kg_nav_frame *d_frames,
                         size_t frame_stride, int cap, int32_t *d_counts);
int kg_nav_push_bits(kg_nav *nav, const uint8_t *bits, size_t chan_stride, const int32_t *nbits, kg_nav_frame *frames, size_t frame_stride,
                     int cap, int32_t *counts);          /* the same on host memory; synchronises */
/* The same from the rows and counts exactly as kg_trk_process_bits_dev leaves them (d_counts_in[ch] records of row ch, -1 - n from a
 * stopped channel = n records; epoch_cap: that call's cap, counts above it are cut to it), nothing going back to the host in between:
 * the nav-bit machine of GPS_Method (e_cpu/kiwi.gps.asm NavSave; every epoch's KG_TRK_INAV flag for E1B, the bit after 19 equal epochs
 * for C/A, a glitch counted as nav_glitch counts it) gives the bits.  Its nav_ms / nav_prev start at 0 at kg_nav_set_mode, so they equal
 * the firmware's when both start at the channel's reset.  Of a record only `flags` is read.  cap >= the bound above with nbits[ch] =
 * epoch_cap (E1B) or ceil(epoch_cap / 20) (C/A).  Enqueue only. */
int kg_nav_push_epochs_dev(kg_nav *nav, const kg_trk_epoch *d_epochs, size_t chan_stride, const int32_t *d_counts_in, int epoch_cap,
                           kg_nav_frame *d_frames, size_t frame_stride, int cap, int32_t *d_counts);
/* holding, the stream index of buf[0], buf[0 .. holding) one byte per bit (room for KG_NAV_MAX_HELD), the bits pushed since
 * kg_nav_set_mode, and nav[3] = nav_ms, nav_prev, nav_glitch.  Synchronises. */
int kg_nav_get_state(kg_nav *nav, int ch, int32_t *holding, uint64_t *bit0, uint8_t *held, uint64_t *pushed, int32_t *nav3);

/* ---------------------------------------------------------------------------
 * Ephemeris decode and satellite position and clock: what reads a validated frame into numbers and what the position solver asks
 * of them.  Frames in (the rows and counts of kg_nav_push_*_dev, on the device), EPHEM out: EPHEM::Subframe with Subframe1..4,
 * LoadPage18 and Valid (gps/ephemeris.cpp:51-110, :218-252) for C/A; decode_page_e1b with decode_word0..6 and 10
 * (gps/GNSS-SDRLIB/sdrnav_gal.cpp:28-286, :327-359) and EPHEM::PageN, Page0..6 (ephemeris.cpp:256-370) for Galileo.  Then, per
 * clock snapshot, LoadAtomic's Valid gate and the per-replica body of LoadFromReplicas (gps/solve.cpp:319-361): SNAPSHOT::GetClock
 * (:168-244), GetClockCorrection, TimeOfEphemerisAge, EccentricAnomaly and GetXYZ (ephemeris.cpp:114-207).
 *
 * The decoded state equals the reference's bit for bit, doubles included:
 *  - rtklib.h's P2_32, P2_33, P2_35, P2_43 and sdrnav_gal.cpp's P2_46 are decimal text that is NOT a power of two as a double (one or
 *    two ulp below): Galileo's e, tgd, OMGd, deln, idot, f1 and A_0G are the raw field times THAT double, then (angles) times SC2RAD,
 *    two roundings left to right.  The C/A fields take exact powers of two (pow(2, -n)).
 *  - gps.h's PI (C/A angles) and rtklib.h's SC2RAD (Galileo angles) are both the text 3.1415926535898, 16 ulp above pi.
 *  - Galileo's week_gst, toes and toc_gst belong to the CHANNEL (CHANNEL::nav.sdreph; CHANNEL::Start clears none of them,
 *    channel.cpp:274-278): words 1 and 4 hand on a t_oe / t_oc only once the channel has seen a week (week_gst != 0), Page1 / Page4 /
 *    Page5 keep the old t_oe / t_oc when handed 0, and a channel bound to another satellite carries its week along.  A satellite's
 *    slot persists in the same way (EPHEM::Init sets only sat and isE1B).  GST weeks up to 2526 (beyond, the reference's int overflows).
 *  - Applied: C/A frames with err == 0 (ParityCheck reaches Ephemeris[sat].Subframe only then); E1B frames with err == 0 or
 *    KG_NAV_ERR_OOS, which decode_word5 raises after Page5 was applied.  SLIP, CRC, ALERT and PARITY frames change nothing.
 * Position and clock pass through sin, cos, atan2 and sqrt, where the device's library and the host's may differ in the last
 * bit: x, y, z within 1e-3 m, ct within 2 ulp, t_k within 2 ulp of t_tx of the reference.
 *
 * Not here: PosSolver and the EKF (kg_pos, below), ionosphere and troposphere, LoadReplicas' glitch guard and include_E1B filter; probation, alert,
 * abort and expecting_preamble (host decisions; the notes carry what bits_tow needs); CHANNEL::Subframe's statistics; tow_time and the
 * L_* debug members; almanac words 7..9.
 * ------------------------------------------------------------------------- */
typedef struct kg_eph kg_eph;
enum { KG_EPH_MAX_SATS = 64,             /* MAX_SATS, gps/gps.h:123 */
       KG_EPH_NAVSTAR = 0, KG_EPH_CA = 1, KG_EPH_E1B = 2,        /* a satellite's kind: Navstar; other C/A (QZSS: page 18 leaves UTC alone); Galileo */
       KG_EPH_SV_NOT_VALID = 1, KG_EPH_SV_POWER = 2, KG_EPH_SV_TOW_DELAYED = 4, KG_EPH_SV_BAD = 8, KG_EPH_SV_TOO_OLD = 16 };
typedef struct {           /* EPHEM's data members as the decode writes them; unsigned as uint32_t */
    uint32_t IODN[4];
    uint32_t IODC, t_oc;
    double   t_gd, a_f[3];
    uint32_t IODE2, t_oe;
    double   C_rs, dn, M_0, C_uc, e, C_us, sqrtA;
    uint32_t IODE3, kind;  /* kind: KG_EPH_* of the last kg_eph_set_sat on this satellite (isE1B) */
    double   C_ic, OMEGA_0, C_is, i_0, C_rc, omega, OMEGA_dot, IDOT;
    double   alpha[4], beta[4];
    uint32_t week, tow, sub, tow_pg;
    double   A_0G, A_1G;
    uint32_t t_0G, WN_0G;
    int32_t  valid, pad_;  /* EPHEM::Valid now */
    uint64_t tow_bit;      /* ours: bit_next of the last frame that updated the TOW, so that bits_tow = bits pushed - tow_bit */
} kg_ephem;
typedef struct {
    int32_t  applied;      /* the frame reached the decode */
    int32_t  tow_updated;  /* nav.tow_updated; 1 for every applied C/A subframe (channel.cpp:827) */
    int32_t  sub, valid;   /* the satellite's sub and Valid after this frame */
    uint32_t tow, week;    /* likewise */
    uint64_t bit_next;     /* the frame's bit + consumed */
} kg_eph_note;
typedef struct { int32_t sat, bits, bits_tow, ms, chips, cg_phase; float power; } kg_eph_snap;    /* SNAPSHOT's inputs */
typedef struct { double x, y, z, ct, t_k; int32_t week, flags; } kg_eph_pos;    /* _sv[0..3], t_k, _week; KG_EPH_SV_* */
int kg_eph_create(kg_ctx *ctx, int nchan, kg_eph **out);  /* 1 <= nchan <= KG_TRK_MAX_CHANS; 64 satellite slots; everything zero, no channel bound */
void kg_eph_destroy(kg_eph *eph);
/* Binds channel ch to satellite slot sat (0 .. 63) of kind KG_EPH_*, as CHANNEL::Start does: the channel keeps its week_gst / toes /
 * toc_gst and the slot its contents; only the slot's kind (and with it valid) is set.  sat = -1 unbinds: the channel's frames are
 * then read and noted with applied = 0.  A satellite bound to another channel: KG_ERR_INVALID.  In stream order, without waiting. */
int kg_eph_set_sat(kg_eph *eph, int ch, int sat, int kind);
int kg_eph_clear_sat(kg_eph *eph, int sat);                /* ours: the slot back to zero (its kind stays).  In stream order */
int kg_eph_clear_chan(kg_eph *eph, int ch);                /* ours: the channel's week_gst, toes, toc_gst back to zero.  In stream order */
/* Reads the rows and counts exactly as kg_nav_push_bits_dev / kg_nav_push_epochs_dev leave them (row ch at d_frames + ch *
 * frame_stride, d_counts[ch] records, cut to 0 .. cap) and applies every applicable frame of every channel, in stream order, to the
 * channel's satellite.  One kg_eph_note per frame read goes to row ch of d_notes (d_notes + ch * note_stride, 8-byte aligned,
 * note_stride >= cap): exactly that many notes are written, nothing else, and the inputs are only read.  Page 18 of Navstar
 * satellites sets the UTC fields, channels in ascending order.  Enqueue only. */
int kg_eph_push_frames_dev(kg_eph *eph, const kg_nav_frame *d_frames, size_t frame_stride, const int32_t *d_counts, int cap,
                           kg_eph_note *d_notes, size_t note_stride);
int kg_eph_push_frames(kg_eph *eph, const kg_nav_frame *frames, size_t frame_stride, const int32_t *counts, int cap,
                       kg_eph_note *notes, size_t note_stride);      /* the same on host memory; synchronises */
int kg_eph_get(kg_eph *eph, int sat, kg_ephem *out);       /* synchronises */
int kg_eph_get_chan(kg_eph *eph, int ch, int32_t *sat, uint32_t *gst3);     /* the bound satellite (-1: none); week_gst, toes, toc_gst.  Synchronises */
int kg_eph_get_utc(kg_eph *eph, int32_t *utc3);            /* gps.delta_tLS, delta_tLSF, tLS_valid.  Synchronises */
/* One kg_eph_pos per snapshot, in the order of LoadFromReplicas: the satellite not Valid (or sat outside 0 .. 63) -> flags =
 * KG_EPH_SV_NOT_VALID; power < 1e5 or > 5e6 (as doubles) -> KG_EPH_SV_POWER; of either only `flags` is written.  Else GetClock with
 * the MAX_TOW_DELAY substitution (KG_EPH_SV_TOW_DELAYED); a bad clock -- E1B only: ms not 0 or 4, chips outside 0 .. 4091 -- gives
 * KG_EPH_SV_BAD and NaN in x, y, z, ct, t_k, as the reference lets NaN run through; t_tx -= GetClockCorrection; ct = C t_tx; t_k;
 * KG_EPH_SV_TOO_OLD when |t_k| / 60 / 60 >= 4; GetXYZ; week.  d_snaps 4-byte, d_out 8-byte aligned.  Enqueue only. */
int kg_eph_sv_dev(kg_eph *eph, const kg_eph_snap *d_snaps, int nsnap, kg_eph_pos *d_out);
int kg_eph_sv(kg_eph *eph, const kg_eph_snap *snaps, int nsnap, kg_eph_pos *out);      /* the same on host memory; synchronises */
/* chips and cg_phase of a snapshot from the 18-bit replica word of kg_trk_get_clocks, by LoadAtomic's masks (solve.cpp:77-79). */
void kg_eph_replica(uint32_t word, int32_t *chips, int32_t *cg_phase);

/* ---------------------------------------------------------------------------------------------------------------------------------
 * The position fix: what turns the rows of kg_eph_sv_dev into a position.  Replaces GNSSDataForEpoch::LoadFromReplicas' compaction
 * (gps/solve.cpp:319-364), SolveTask's three solvers and its per-epoch statements (solve.cpp:571-578, :616-639), PosSolverImpl
 * (gps/PosSolver.cpp:32-38, :45-59, :64-144, :169-172), SinglePointPositionSolver.h:20-64, EKFPositionSolver.h:21-124,
 * PositionSolverBase.h:61-125, Ellipsoid.h:39-63, TNT's matmult / mean / norm / makeDiag and JAMA's LU (pkgs/TNT_JAMA), and of
 * update_gps_info_after the lines :497-516 (grn_yel_red, ch_has_soln, az/el).  Not here: clock_correction, tod_correction, the gps.*
 * tables (az / el[last_samp], shadow_map, fix counters, POS_data / MAP_data), the "already have az/el" skip, the glitch counters,
 * compute_dop.  DESIGN.md 6.13.
 *
 * An epoch is nrow rows, row r = channel r: a kg_eph_snap, of which sat and power are read, and the kg_eph_pos kg_eph_sv_dev made of it.  Rows
 * with KG_EPH_SV_NOT_VALID, and rows whose bit is set in the epoch's `skip` word (the host's glitch guard and include_E1B filter), were
 * never in Replicas; KG_EPH_SV_POWER rows advance the reference's `i` but do not enter; every other row enters, NaN rows included.
 * The type of an entering row is kinds[_sat[i]] with the reference's index quirk (see kg_pos.h, load_epoch).  An epoch with no row in
 * Replicas changes nothing (`if (good == 0) continue;`); its record reports the held state. */
typedef struct kg_pos kg_pos;
enum { KG_POS_CALLED = 1,                /* solve() ran on a non-empty set this epoch */
       KG_POS_POS_VALID = 2, KG_POS_SPP_VALID = 4, KG_POS_EKF_VALID = 8 };      /* pos_valid(), spp_valid(), ekf_valid() after the epoch */
typedef struct { double x, y, z, t_rx, osc_corr, lambda, phi, alt; int32_t flags, ekf_running, nsv, pad; } kg_pos_fix;   /* pos(), t_rx(), osc_corr(), llh() */
typedef struct { double elev_deg, azim_deg; int32_t sat, ch, type, week, el, az; } kg_pos_sat;   /* el = az = 0: rejected by solve.cpp:515 or no fix */
typedef struct { kg_pos_fix fix[3]; kg_pos_sat sat[12]; int32_t chans, grn_yel_red; uint32_t ch_has_soln, pad; } kg_pos_epoch;
typedef struct {                         /* one solver: PosSolverImpl's members with its two solvers' */
    double spp_state[4], spp_cov[16], ekf_state[5], ekf_P[25];
    double pos[3], t_rx, osc_corr, lambda, phi, alt, ct_rx[2];
    uint64_t ticks_spp[2], ticks_ekf[2];
    int32_t pos_valid, ekf_running, state_spp[2], ekf_valid, pad;      /* ekf_valid: EKFPositionSolver::_valid */
} kg_pos_state;
/* kinds: KG_EPH_* per satellite slot (Sats[].type).  uere, f_osc: PosSolver::make's arguments (the reference: UERE 6.0, ADC_CLOCK_TYP
 * 124.9999e6), finite and positive.  Three fresh solvers (TNT's unset _state / _cov are zero here), use_kalman 1, plot_e1b 0. */
int kg_pos_create(kg_ctx *ctx, const int32_t kinds[64], double uere, double f_osc, kg_pos **out);
void kg_pos_destroy(kg_pos *pos);
int kg_pos_set_mode(kg_pos *pos, int use_kalman, int plot_e1b);        /* admcfg's two switches (solve.cpp:618-619); in stream order */
int kg_pos_reset(kg_pos *pos);                                         /* ours: three fresh solvers; the mode stays.  In stream order */
/* nepoch epochs in order, one launch: epoch e reads rows e * nrow .. e * nrow + nrow - 1 of d_snaps and d_sv, d_ticks[e] (the 48-bit
 * ADC tick count) and, if d_skip is given, d_skip[e]; writes d_out[e].  1 <= nrow <= KG_TRK_MAX_CHANS, 1 <= nepoch <= 65536;
 * d_snaps and d_skip 4-byte, d_sv, d_ticks and d_out 8-byte aligned; anything else KG_ERR_INVALID, nothing done.  Enqueue only. */
int kg_pos_solve_dev(kg_pos *pos, const kg_eph_snap *d_snaps, const kg_eph_pos *d_sv, int nrow, int nepoch, const uint64_t *d_ticks,
                     const uint32_t *d_skip, kg_pos_epoch *d_out);
int kg_pos_solve(kg_pos *pos, const kg_eph_snap *snaps, const kg_eph_pos *sv, int nrow, int nepoch, const uint64_t *ticks,
                 const uint32_t *skip, kg_pos_epoch *out);              /* the same on host memory; synchronises */
int kg_pos_get_state(kg_pos *pos, int solver, kg_pos_state *out);       /* solver 0 .. 2 (all, not Galileo, only Galileo); synchronises */

/* kg_fir_process_dev plus the extension taps of ProcessData (SURVEY.md 8(f) rank 4;
 * rx/CuteSDR/fastfir.cpp:278-302): for block b of list entry i, 1024 complex floats at
 * d_pre / d_post + i*tap_stride + b*1024 (either may be NULL): pre = the forward spectrum
 * times the CIC compensation table (what receive_FFT(PRE_FILTERED) is handed), post = the
 * filtered spectrum (receive_FFT(POST_FILTERED), specAF_FFT).  A PRE_FILTERED extension that
 * edits the buffer (the `buf_modified` path, :286-290) is not supported on this path.  The
 * other taps of c2s_sound() are plain buffers of this API: receive_iq_pre_fir = the unpack
 * output, receive_iq_pre_agc = the FIR output (an iq_buf_t ring when d_out walks
 * [N_DPBUF][512]), receive_iq_post_agc / receive_real / receive_S_meter = kg_post outputs.
 * Written: 8 * 1024 * (nout[i] / 512) bytes of row i of each tap given (8-byte aligned, tap_stride in complex samples). */
int kg_fir_process_taps_dev(kg_fir *fir, const int32_t *chans, int nch, const void *d_in, size_t in_stride, int n,
                            void *d_out, size_t out_stride, int32_t *nout, void *d_pre, void *d_post,
                            size_t tap_stride);

/* A PRE_FILTERED extension that EDITS the spectrum it is handed (`buf_modified`, fastfir.cpp:286-290):
 * after kg_fir_process_taps_dev() delivered d_pre, the caller rewrites those 1024-point blocks on the
 * device and calls this.  Block b (b < nblk[i]) of list entry i is filtered again as the reference
 * filters a modified buffer -- m_pFilterCoef (the coefficients WITHOUT the CIC compensation) times the
 * edited block, backward transform, samples 512..1023 -- into d_out + i*out_stride + 512 b, replacing
 * what kg_fir_process_taps_dev wrote there.  The un-compensated coefficients are those kg_fir_setup
 * designed, or what kg_fir_set_coef_plain handed over.  Enqueue only.  d_pre and d_out: 8-byte aligned; 1024 * nblk[i] samples of
 * row i read, 512 * nblk[i] written. */
int kg_fir_refilter_dev(kg_fir *fir, const int32_t *chans, int nch, const int32_t *nblk, const void *d_pre,
                        size_t tap_stride, void *d_out, size_t out_stride);
/* m_pFilterCoef[1024] (complex float) for kg_fir_refilter_dev when kg_fir_set_coef supplied
 * m_pFilterCoef_CIC; kg_fir_set_coef alone uses the same array for both. */
int kg_fir_set_coef_plain(kg_fir *fir, int ch, const float *coef_fft);

/* ---------------------------------------------------------------------------
 * The audio spectrum display, `SET spc_=2` (SPEC_SND_AF): specAF_FFT (rx/rx_sound.cpp:175-220), called from inside
 * CFastFIR::ProcessData with the filtered spectrum of every completed block (rx/CuteSDR/fastfir.cpp:251-253, :301-302).  A row is
 * 1024 bytes: per bin pwr = re * re (the real part only, :198), dB = 10.0 * log10f(pwr * scale + 1e-30) clamped to [-200, 0] and
 * decremented, (u1_t) (int) dB stored at bin ^ 512 (:208-216); scale = 10 * 2 / (CUTESDR_MAX_VAL^2 * 1024^2) times 1e6 for the
 * passband filter's rows and times 0.0004 for the channel-null filter's (:201-202).  Bytes span 55 (a zero bin) .. 255.  The device's
 * log10f is the host libm's bit for bit, so a row is an exact function of the spectrum (csrc/kg_spec.h is the one definition for
 * both).  NaN input is outside the contract ((int) NaN is undefined in the reference); +-inf and overflow give byte 255. */
enum { KG_SPEC_PASSBAND = 0, KG_SPEC_CHAN_NULL = 1 };      /* SND_INSTANCE_FFT_PASSBAND, SND_INSTANCE_FFT_CHAN_NULL, rx/rx_sound.h:34-35 */
#define KG_SPEC_ROW 1024                                   /* FFT_WIDTH, rx_sound.cpp:180 */
/* Row r from the 1024 complex floats at d_spec + r*spec_stride (complex samples; what kg_fir_process_taps_dev wrote to d_post)
 * with the scale of inst[r] (KG_SPEC_*), to d_rows + r*row_stride (bytes; d_rows and row_stride multiples of 4; d_spec 8-byte
 * aligned).  1024 bytes of every row are written.  Enqueue only. */
int kg_snd_spec_rows_dev(kg_ctx *ctx, const void *d_spec, size_t spec_stride, int nrows, const int32_t *inst, void *d_rows,
                         size_t row_stride);
/* "limit update rate" (rx_sound.cpp:186-195), host only, the clock is the caller's: returns 1 when a row handed over at now_ms is to
 * be sent (snd_send_msg_data, :218).  Fires only when now_ms > *last_ms + 125; then *last_ms += 125 if it is non-zero, else
 * *last_ms = now_ms.  With *last_ms = 0 at the start of a connection the first call fires only when now_ms > 125. */
int kg_snd_spec_due(uint32_t *last_ms, uint32_t now_ms);
/* kg_fir_process_each_dev plus the row of every completed block, formed from the registers that hold the filtered spectrum
 * (fastfir.cpp:293 -> :301-302): block b of list entry i at d_rows + i*row_stride + 1024 b with the scale of inst[i] (on a receiver
 * bank's objects: row chans[i], like every caller-visible buffer there).  d_post / tap_stride as in kg_fir_process_taps_dev (may be
 * NULL / 0): the same values the bytes were formed from.  d_out may be NULL -- the OutBuf == NULL call of fastfir.cpp:306, the
 * channel-null filter's (rx_sound.cpp:804): no backward transform, history and FirPos() advance as with an output buffer, and
 * nout[i] / 512 still says how many blocks (rows) entry i completed.  No spectrum goes to memory unless d_post is given.
 * d_rows and row_stride: multiples of 4 bytes; the complex-float buffers as in kg_fir_process_dev.  Written: 1024 * (nout[i] / 512)
 * bytes of row i of d_rows, 8 * nout[i] of d_out, 8 * 1024 * (nout[i] / 512) of d_post.  Enqueue only. */
int kg_fir_process_spec_dev(kg_fir *fir, const int32_t *chans, int nch, const void *d_in, size_t in_stride,
                            const int32_t *n_each, void *d_out, size_t out_stride, int32_t *nout, void *d_rows,
                            size_t row_stride, const int32_t *inst, void *d_post, size_t tap_stride);

/* ---------------------------------------------------------------------------
 * The FFT extension (extensions/FFT/FFT.cpp), the one consumer of receive_FFT(POST_FILTERED): fft_msgs (:193-261) and fft_data
 * (:69-191) over the filtered spectrum of every completed CFastFIR block (what kg_fir_process_taps_dev / kg_fir_process_spec_dev
 * leave in d_post).  Three functions (:66): wf, a waterfall line per block; spec, a spectrum whose sending is limited to one per
 * 100 ms; integ, the integrator -- the passband power folded into up to 200 time bins of 1024 sums over a period the user sets, a
 * line per block.  A row is 1024 bytes: per column pwr -- re * re of this block outside integ (the real part only, :116), the bin's
 * running sum of re * re + im * im under it (:127-139) -- then 10.0 * log10f(pwr * scale + 1e-30) clamped to [-200, 0], decremented,
 * (u1_t) (int), stored at column ^ 512 (:157-167).  The 1025-byte message of :188 is the row's bin followed by the row.
 * A column's sum is added to in block order, one addition per block, and the device's log10f is the host libm's bit for bit: sums and
 * rows are an exact function of the spectra (csrc/kg_fftext.h is the one definition for device and host).  NaN input is outside the
 * contract as for the audio spectrum rows; +-inf and overflow give byte 255.
 * The schedule (:72-101: which instance, the latched reset, the bin of a block, the blocks dropped at bin >= 200) depends on no
 * sample: it runs on the host, nothing here synchronises but the calls that say so.
 *   kg_fftext_create    nchan channels (1 .. 1024), each with 200 x 1024 float sums (800 KiB of device memory) and ncma[200]; a
 *                       channel starts like a fresh connection: function off, time 0, nothing latched, sums zero.
 *   kg_fftext_set_rate  what ext_update_get_sample_rateHz answers (:79), a double; finite and above 0, else KG_ERR_INVALID.
 *   kg_fftext_set_run   `SET run=%d` (:206-244); is_sam / is_qam: snd->isSAM and snd->mode == MODE_QAM AT THE COMMAND.  Chooses the
 *                       instance (KG_SPEC_CHAN_NULL only for KG_FFTEXT_SPEC while is_sam) and the scale: (float) (20.0 / (float)
 *                       (32767^2 * 1024^2)) times 1e4 (wf, integ), 1e6 (spec) or 100 (spec while is_sam); zeroes the limiter's
 *                       last_ms under spec.  Does NOT latch a reset: the sums of the function before carry over, as in the
 *                       reference.  run outside -1 .. 2: KG_ERR_INVALID, nothing changed.
 *   kg_fftext_set_itime `SET itime=%lf` (:246-252): stores the period and latches a reset.  Any double is stored.
 *   kg_fftext_clear     `SET clear` (:254-258): latches a reset.
 *   kg_fftext_restart   ours: the channel as kg_fftext_create left it (a new connection); the sums are zeroed by the next call that
 *                       takes a block of it, or read as zero by kg_fftext_state.
 * A latched reset is applied ahead of the first block of the channel's instance (:78-90): fft_sec = 1.0 / (rate * 2 / 1024), bins =
 * trunc(time / fft_sec), fi = 0, sums and ncma zeroed.  Under integ the block's bin is trunc(fmod(fi, time) / time * bins), then
 * fi += fft_sec, and a block whose bin is 200 or more is dropped (:92-98); otherwise the bin is 0. */
typedef struct kg_fftext kg_fftext;
enum { KG_FFTEXT_OFF = -1, KG_FFTEXT_WF = 0, KG_FFTEXT_SPEC = 1, KG_FFTEXT_INTEG = 2 };     /* FUNC_*, FFT.cpp:66 */
#define KG_FFTEXT_ROW 1024                                 /* INTEG_WIDTH, FFT.cpp:33 */
#define KG_FFTEXT_MAX_BINS 200                             /* MAX_BINS, FFT.cpp:38 */
#define KG_FFTEXT_UPDATE_MS 100                            /* UPDATE_MS, FFT.cpp:177 */
typedef struct kg_fftext_info {
    int32_t run, instance;                 /* KG_FFTEXT_*, KG_SPEC_* */
    float fft_scale, spectrum_scale;
    int32_t bins, reset;                   /* reset: 1 while a reset is latched */
    uint32_t last_ms;
    int32_t reserved;
    double fi, fft_sec, time;
} kg_fftext_info;
int kg_fftext_create(kg_ctx *ctx, int nchan, kg_fftext **out);
void kg_fftext_destroy(kg_fftext *fx);
int kg_fftext_set_rate(kg_fftext *fx, double sample_rate);
int kg_fftext_set_run(kg_fftext *fx, int ch, int run, int is_sam, int is_qam);
int kg_fftext_set_itime(kg_fftext *fx, int ch, double itime);
int kg_fftext_clear(kg_fftext *fx, int ch);
int kg_fftext_restart(kg_fftext *fx, int ch);
/* fft_data for nblk[i] blocks of channel chans[i] from the filter of instance inst[i] (KG_SPEC_*), entries in list order, a
 * channel's blocks in block order (a channel may be listed more than once: passband and channel-null blocks interleaved): block b of
 * entry i is the 1024 complex floats at d_spec + 2 * (i*spec_stride + 1024 b) (spec_stride in complex samples; d_spec 8-byte
 * aligned).  Every block the schedule takes gives one row, numbered from 0 in that order: row r at d_rows + r*row_stride (d_rows and
 * row_stride multiples of 4 bytes, row_stride >= 1024), and, on the host and without a sync, its channel, its list entry, the
 * block's index within that entry and its bin in rx_of_row / ent_of_row / blk_of_row / bin_of_row[r] (max_rows entries each, any may
 * be NULL).  Returns the number of
 * rows.  ONE kernel launch (none when no block is taken and nothing is to be zeroed).  1 <= nch <= 65536, 0 <= nblk[i] <= 4096.
 * Refused, with nothing changed and nothing enqueued: KG_ERR_INVALID for an argument out of range or more rows than max_rows;
 * KG_ERR_STATE for what the reference leaves undefined -- no rate set, an integ block while the period is not finite or not above 0
 * (fmod(fi, 0) is NaN and (int) of it indexes pwr), a reset whose time / fft_sec does not fit an int.
 * Read: 8 * 1024 * nblk[i] bytes of row i of d_spec.  Written: 1024 bytes of each of the returned number of rows.  Enqueue only. */
int kg_fftext_process_dev(kg_fftext *fx, const int32_t *chans, int nch, const int32_t *nblk, const int32_t *inst, const float *d_spec,
                          size_t spec_stride, uint8_t *d_rows, size_t row_stride, int max_rows, int32_t *rx_of_row, int32_t *ent_of_row,
                          int32_t *blk_of_row, int32_t *bin_of_row);
/* the same on host memory; synchronises */
int kg_fftext_process(kg_fftext *fx, const int32_t *chans, int nch, const int32_t *nblk, const int32_t *inst, const float *spec,
                      size_t spec_stride, uint8_t *rows, size_t row_stride, int max_rows, int32_t *rx_of_row, int32_t *ent_of_row,
                      int32_t *blk_of_row, int32_t *bin_of_row);
/* "limit spectrum update rate" (:174-186), host only, the clock is the caller's: 1 when the row of a block handed over at now_ms is
 * to be sent (ext_send_msg_data, :188), 0 when it is held back.  Only KG_FFTEXT_SPEC is limited: fires when now_ms > last_ms + 100;
 * then last_ms += 100 if it is non-zero, else last_ms = now_ms.  Call it once per row, in row order. */
int kg_fftext_due(kg_fftext *fx, int ch, uint32_t now_ms);
/* Channel ch's state; pwr (200 x 1024 floats) and ncma (200) may be NULL.  With pwr it synchronises. */
int kg_fftext_state(kg_fftext *fx, int ch, kg_fftext_info *info, float *pwr, int32_t *ncma);

/* The IQ display extension (extensions/IQ_display/iq_display.cpp with rx/kiwi/pll.h), a consumer of receive_iq_samps(PRE_AGC): the
 * CFastFIR output of every sound block (kg_fir_process_dev's d_out; none while the receiver is in NBFM).  The constellation in
 * points mode (per ring entry the byte pairs of the sample that was there and of the new one, a row of points * 4 bytes whenever the
 * ring comes round) and in density mode (a row of points * 2 bytes from the map both instances share); carrier recovery by a
 * second-order PLL on the sample raised to a power (1 / 2 / 4 / 8: BPSK .. 8PSK) or by two PLLs on its square (MSK); the running
 * complex mean and amplitude mean, and the four numbers of the text message (cmaI, cmaQ, df, phase).  Every byte and every float
 * is an exact function of the samples: csrc/kg_iqd.h is the one definition for device and host, the device's sinf / cosf / atan2f /
 * fmodf / hypotf are the host libm's bit for bit.  NaN or infinite samples, and overflow inside the power (|s|^8 needs |s| < 6e4),
 * are outside the contract.
 * The schedule (ring positions, rows, maN, nsamp -- :71-111) depends on no sample: it runs on the host, and nothing here synchronises
 * but the calls that say so.  Commands take effect between calls, in call order.
 *   kg_iqd_create            nchan channels (1 .. 1024), 416 KiB of device memory each (_iq, _plot, _map) plus the scalars
 *   kg_iqd_init              `SET ext_server_init`: the constructor's state (points 1024, exponent 1, 12 kHz, bandwidth 10, gain auto,
 *                            every array zero).  Every other call on a channel needs it first (KG_ERR_STATE).
 *   kg_iqd_set_run           `SET run=%d`: run != 0 is set_sample_rate((float) rate) -- maNsend = fs / 4 and the three PLLs re-initialised,
 *                            nothing else; rate as ext_update_get_sample_rateHz answers (1 .. 1e9, else KG_ERR_INVALID).
 *   kg_iqd_set_gain          `SET gain=%d`: (float) pow(10.0, ((float) gain - 50) / 10.0), 0 for auto
 *   kg_iqd_set_points        `SET points=%d`; outside 1 .. 16384 KG_ERR_INVALID (the reference leaves its arrays or sends a negative length)
 *   kg_iqd_set_pll_mode      `SET pll_mode=%d arg=%d`: <= 1: exponent = arg (0: PLL off), MSK off; 2: exponent 2, MSK on, baud = arg; all
 *                            re-initialise the PLLs.  A negative exponent is KG_ERR_INVALID: not ported (its division is libgcc's).
 *   kg_iqd_set_pll_bandwidth / kg_iqd_set_draw (0 points, 1 density, anything else: no sample is processed) / kg_iqd_set_display_mode
 *                            (0 multiplies by the carrier, anything else shows the carrier) / kg_iqd_clear (`SET clear`: cma, ama, maN,
 *                            nsamp, the PLLs; the rings stay) */
typedef struct kg_iqd kg_iqd;
enum { KG_IQD_POINTS = 0, KG_IQD_DENSITY = 1 };            /* IQ_POINTS, IQ_DENSITY, iq_display.cpp:21-22 */
enum { KG_IQD_MATH_HYPOTF = 0, KG_IQD_MATH_FMODF = 1 };
#define KG_IQD_RING 16384                                  /* N_IQ_RING, iq_display.cpp:25 */
#define KG_IQD_MAX_NS 512
typedef struct kg_iqd_status {             /* what the text message of :108 carries */
    float cmaI, cmaQ;
    double df;
    float phase;
    int32_t reserved;
} kg_iqd_status;
typedef struct kg_iqd_row {                /* one ext_send_msg_data of :82 / :93 */
    int32_t ch, ent, blk, samp;            /* channel, list entry, block within the entry, the sample behind which the row went out */
    int32_t cmd, len;                      /* (draw << 1) + instance; points * 4 or points * 2 bytes */
    int64_t off;                           /* from d_rows */
} kg_iqd_row;
typedef struct kg_iqd_info {
    int32_t inited, run, points, nsamp, exponent, msk_mode, msk_baud, draw, display_mode, maN, maNsend, ring[2], reserved;
    float gain, fs, pll_bandwidth, cmaI, cmaQ, ama;
    float pll[3][7];                       /* _pll, _pllMinus, _pllPlus: fs, fc, df, phase, b[0], b[1], ud */
} kg_iqd_info;
int kg_iqd_create(kg_ctx *ctx, int nchan, kg_iqd **out);
void kg_iqd_destroy(kg_iqd *q);
int kg_iqd_init(kg_iqd *q, int ch);
int kg_iqd_set_run(kg_iqd *q, int ch, int run, double rate);
int kg_iqd_set_gain(kg_iqd *q, int ch, int gain);
int kg_iqd_set_points(kg_iqd *q, int ch, int points);
int kg_iqd_set_pll_mode(kg_iqd *q, int ch, int pll_mode, int arg);
int kg_iqd_set_pll_bandwidth(kg_iqd *q, int ch, float bandwidth);
int kg_iqd_set_draw(kg_iqd *q, int ch, int draw);
int kg_iqd_set_display_mode(kg_iqd *q, int ch, int display_mode);
int kg_iqd_clear(kg_iqd *q, int ch);
/* display_data for nblk[i] blocks of ns samples (1 .. 512) of channel chans[i] as instance inst[i] (0 / 1: the `ch` of the class; the
 * call site of rx_sound.cpp passes 0), entries in list order, a channel's blocks in block order (a channel may be listed more than
 * once): block b of entry i is the ns complex floats at d_iq + 2 * (i*iq_stride + ns*b) (iq_stride in complex samples; d_iq 8-byte
 * aligned).  Rows are packed back to back into d_rows (16-byte aligned, rows_cap bytes) in the order the reference sends them;
 * row_map[r] (max_rows entries; may be NULL) says whose row r is, where it is and how long.  The k-th block of the call (list order)
 * leaves its status record in d_status[k] (8-byte aligned, status_cap records) and, on the host, status_sent[k] (may be NULL): 1
 * when the reference sends the text message behind that block (nsamp > maNsend).  Returns the number of rows.  ONE kernel launch.
 * 1 <= nch <= 4096, 0 <= nblk[i] <= 4096, at most 8192 blocks a call.
 * Refused, with nothing changed and nothing enqueued: KG_ERR_INVALID for an argument out of range (ns, an instance), more row bytes
 * than rows_cap, more rows than max_rows, more blocks than status_cap; KG_ERR_STATE for a channel without kg_iqd_init or without a
 * sample rate (kg_iqd_set_run with run != 0).
 * Read: 8 * ns * nblk[i] bytes of row i of d_iq.  Written: the bytes the row map names, one status record per block.  Enqueue only. */
int kg_iqd_process_dev(kg_iqd *q, const int32_t *chans, int nch, const int32_t *nblk, const int32_t *inst, int ns, const float *d_iq, size_t iq_stride,
                       uint8_t *d_rows, size_t rows_cap, kg_iqd_status *d_status, size_t status_cap, kg_iqd_row *row_map, int max_rows,
                       int32_t *status_sent);
/* the same on host memory (row_map is needed); synchronises */
int kg_iqd_process(kg_iqd *q, const int32_t *chans, int nch, const int32_t *nblk, const int32_t *inst, int ns, const float *iq, size_t iq_stride,
                   uint8_t *rows, size_t rows_cap, kg_iqd_status *status, size_t status_cap, kg_iqd_row *row_map, int max_rows, int32_t *status_sent);
/* Channel ch's whole state, for tests: iq (2 x 16384 complex floats), plot (2 x 16384 x 4 bytes) and map (16384 x 2 bytes) may be NULL.
 * Synchronises. */
int kg_iqd_state(kg_iqd *q, int ch, kg_iqd_info *info, float *iq, uint8_t *plot, uint8_t *map);
/* d_out[i] = hypotf(d_a[i], d_b[i]) (KG_IQD_MATH_HYPOTF: std::abs of a complex float) or fmodf(d_a[i], d_b[i]) (KG_IQD_MATH_FMODF: the
 * PLL's phase wrap) as the device code of kg_iqd computes them: the host libm's values, bit for bit (tests/test_iqd_gpu.py).  4-byte
 * aligned arrays of n floats.  Enqueue only. */
int kg_iqd_math_dev(kg_ctx *ctx, int fn, const float *d_a, const float *d_b, size_t n, float *d_out);

/* The Loran-C extension (extensions/Loran_C/loran_c.cpp), the second consumer of receive_iq_samps(PRE_AGC): the CFastFIR output of
 * every sound block (none while the receiver is in NBFM).  The power of every sample is folded into time buckets that cover one Group
 * Repetition Interval (GRI) of a Loran-C chain -- bucket bn = floor(fmod(samp - offset, samp_per_GRI)) --, for two chains (Loran
 * channels 0 and 1) at once, each under one of three averaging rules (CMA with a time-out, EMA, IIR); whenever a channel comes to
 * bucket 0 with more than i_srate samples behind its last row, its averages go out as a row of nbucket + 1 bytes, the "scope".
 * Every byte and every float is an exact function of the samples: csrc/kg_lorc.h is the one definition for device and host, in the
 * reference's operand types, and the device's expf is the host libm's bit for bit.  Samples are finite with |re|, |im| <= 3e4.
 * The schedule (buckets, rows, clears, navgs) depends on no sample: it runs on the host, and nothing here synchronises but the calls
 * that say so.  Commands take effect between calls, in call order.  What the reference does not define is refused with
 * KG_ERR_INVALID, nothing changed: a Loran channel outside 0 .. 1; a gri outside 1 .. 9999; a gri whose nbucket -- floor(srate * gri /
 * 1e5) + 1, halved with samp_per_GRI when above 1199 -- is 1199 or more (the reference then writes one past its scope[] array: GRI
 * 9990 at 12 kHz); an offset before the channel has a GRI; an avg_algo outside 0 .. 2; and, at the push, a started connection one of
 * whose channels has no GRI, is under EMA with lround(avg_param) < 1 or under IIR with a negative or non-finite avg_param.  Every
 * other call on a connection needs kg_lorc_init first (KG_ERR_STATE). */
typedef struct kg_lorc kg_lorc;
enum { KG_LORC_CMA = 0, KG_LORC_EMA = 1, KG_LORC_IIR = 2 };                /* AVG_CMA, AVG_EMA, AVG_IIR, loran_c.cpp:58-60 */
enum { KG_LORC_SCOPE_DATA = 0, KG_LORC_SCOPE_RESET = 1 };                  /* loran_c.cpp:17-18 */
#define KG_LORC_MAX_GRI 9999                               /* loran_c.cpp:23 */
#define KG_LORC_MAX_BUCKET 1199                            /* loran_c.cpp:24 */
#define KG_LORC_MAX_NS 512
typedef struct kg_lorc_row {               /* one ext_send_msg_data of :119-120 */
    int32_t conn, blk, samp, ch;           /* connection, block of its entry, sample of the block the row went out AHEAD of, Loran channel */
    int32_t cmd, len;                      /* KG_LORC_SCOPE_RESET for the first row behind a `SET gri` or `SET start`, else _DATA; nbucket + 1 */
    int64_t off;                           /* from the rows' first byte; a multiple of 16 */
} kg_lorc_row;
typedef struct kg_lorc_chan {              /* loran_c_ch_t, :29-39, without avg[] */
    uint32_t gri, samp, nbucket, dsp_samps, avg_samps, navgs;
    double samp_per_GRI;
    float gain, max;
    int32_t offset, avg_algo;
    double avg_param_f;
    int32_t avg_param_i, restart;
} kg_lorc_chan;
typedef struct kg_lorc_info {              /* loran_c_t, :41-52 */
    int32_t inited, started;
    uint32_t i_srate;
    int32_t redraw_legend;
    double srate;
    kg_lorc_chan ch[2];
} kg_lorc_info;
/* nconn (1 .. 1024) objects of loran_c[] (:54), 9.4 KiB of device memory each (avg[2][1199], max) */
int kg_lorc_create(kg_ctx *ctx, int nconn, kg_lorc **out);
/* the object with its connections (the extension's close; loran_c.cpp:54 is static) */
void kg_lorc_destroy(kg_lorc *q);
/* `SET ext_server_init` (:218-228): the memset; srate is what ext_update_get_sample_rateHz answers (1 .. 1e9), i_srate is snd_rate
 * (>= 0).  Whether the connection is started stays: the registration is not part of the struct. */
int kg_lorc_init(kg_lorc *q, int conn, double srate, int i_srate);
/* `SET gri%d=%d` (:230-240) with init_gri (:198-208): samp_per_GRI, nbucket, the halving; redraw_legend and restart set */
int kg_lorc_set_gri(kg_lorc *q, int conn, int ch, int gri);
/* `SET offset%d=%d` (:242-250): (offset + delta) % nbucket with the int sum converted to unsigned first -- not the residue of a
 * negative sum; restart set */
int kg_lorc_set_offset(kg_lorc *q, int conn, int ch, int offset);
/* `SET gain%d=%d` (:252-260): (float) pow(10.0, ((float) -gain) / 10.0), 0 for auto; restart set */
int kg_lorc_set_gain(kg_lorc *q, int conn, int ch, int gain);
/* `SET avg_algo%d=%d` (:262-269): KG_LORC_CMA / _EMA / _IIR; restart set */
int kg_lorc_set_avg_algo(kg_lorc *q, int conn, int ch, int avg_algo);
/* `SET avg_param%d=%lf` (:271-280): avg_param_f and avg_param_i = lround(avg_param); restart set */
int kg_lorc_set_avg_param(kg_lorc *q, int conn, int ch, double avg_param);
/* `SET start` (:282-292): redraw_legend and both restarts set, loran_c_data registered */
int kg_lorc_start(kg_lorc *q, int conn);
/* `SET stop` (:294-302): unregistered; the state is kept, as the reference keeps it */
int kg_lorc_stop(kg_lorc *q, int conn);
/* loran_c_data (:65-196) for nblk[i] blocks (0 .. 256) of ns samples (1 .. 512) of connection conns[i] (each at most once), on HOST
 * arrays: block b of entry i is the ns complex floats at iq + 2 * (i*iq_stride + ns*b) (iq_stride in complex samples).  A connection
 * that is not started takes nothing (its callback is not registered).  Rows go to rows + row_map[r].off in the reference's send order
 * -- per connection in list order, sample-major, channel 0 ahead of channel 1 on the same sample --, each at the next multiple of 16;
 * the bytes between them stay as they are.  *nrows: how many.  ONE kernel launch.  Refused with nothing changed and nothing enqueued:
 * an argument out of range, more row bytes than rows_cap, more rows than max_rows, and the pushes named above.  Synchronises. */
int kg_lorc_process(kg_lorc *q, const int32_t *conns, int nconn, const int32_t *nblk, int ns, const float *iq, size_t iq_stride,
                    uint8_t *rows, size_t rows_cap, kg_lorc_row *row_map, int max_rows, int32_t *nrows);
/* The schedule of that push (:85-88, :121-146: buckets, rows, clears -- no sample enters it), walked on copies: how many runs it has
 * (maximal stretches of samples over which the bucket rises by one a sample; the kernel's table holds one entry each), how many rows
 * it sends and the bytes from the rows' first byte to the last row's end -- what `rows` must hold.  Any of the three may be NULL.
 * Changes nothing, enqueues nothing; refuses what the push refuses, but for the capacities. */
int kg_lorc_plan(kg_lorc *q, const int32_t *conns, int nconn, const int32_t *nblk, int ns, int32_t *nruns, int32_t *nrows, size_t *row_bytes);
/* Connection conn's whole state (loran_c_t, :29-52), for tests: every scalar of both channels and avg[2][1199] (may be NULL).
 * Synchronises. */
int kg_lorc_state(kg_lorc *q, int conn, kg_lorc_info *info, float *avg);
/* the number of the `EXT ms_per_bin=` line (:223-225): float(1.0 / srate * 1e3), doubled in float when i_srate > 12000 */
float kg_lorc_ms_per_bin(double srate, int i_srate);

/* ---- The FAX extension (extensions/FAX/FaxDecoder.cpp, FaxDecoder.h, fax.cpp): HF weather fax from the 16-bit mono audio a sound block
 * ends as (receive_real_samps, rx/rx_sound.cpp:1100-1111) -- the other tap of c2s_sound().  Per audio sample a quadrature mix, two
 * 17-tap FIR filters, a normalisation and a phase-difference discriminator; per line two single-frequency Fourier sums (start and stop
 * tone), a wedge search (phasing), a resample to imagewidth pixels and a blend of successive lines.  Every row byte and every decision
 * is an exact function of the samples: csrc/kg_fax.h is the one definition for device and host, in the reference's operand types.
 *
 * The SCHEDULE depends on the samples (the phasing result moves every later line boundary, the stop tone suppresses rows), so the whole
 * FaxDecoder of a connection lives on the device and a push's outputs carry counts the DEVICE writes: for entry i of the list, with
 * max_lines the capacity the caller chose (kg_fax_max_lines gives the least one),
 *   counts[4*i]      rows sent;  counts[4*i + 1]  lines completed;  counts[4*i + 2]  1 if a capacity was exceeded (never, by the bound)
 *   rows + (i*max_lines + r) * row_stride     row r: KG_FAX_MSG_DRAW, then imagewidth bytes (ext_send_msg_data, :404)
 *   recs + i*max_lines + l                    line l (kg_fax_rec)
 * Defined here where the reference leaves it open: what `new` and kiwi_imalloc hand out is zeros (so the line a row is blended with
 * behind lines that autostop counted without decoding is zeros); a pixel whose discriminator is NaN (silence) is byte 0.
 * Refused with nothing changed: lpm < 1, deviation 0, a bandwidth outside 0 .. 2, imagewidth < 1, fewer samples a line than
 * imagewidth, more than KG_FAX_MAX_SPL samples a line, a nominal rate outside 1 .. 1e6 Hz, a sample rate outside half to twice the
 * nominal, a shift that is negative, above 1 or not finite.  Not ported: the pgm file, the shell commands, fax_task's sequence numbers. */
typedef struct kg_fax kg_fax;
#define KG_FAX_MAX_SPL 24576                               /* samples a line: 60 lpm at 20250 Hz is 20250 */
#define KG_FAX_BLK 512                                     /* FASTFIR_OUTBUF_SIZE, fax.cpp:85 */
#define KG_FAX_MSG_DRAW 254                                /* FaxDecoder.h:34 */
enum { KG_FAX_IMAGE = 0, KG_FAX_START = 1, KG_FAX_STOP = 2 };              /* FaxDecoder.h:102 */
enum { KG_FAX_SPS_CHANGED = 1, KG_FAX_AUTOSTOPPED_0 = 2, KG_FAX_AUTOSTOPPED_1 = 4, KG_FAX_PHASED = 8,     /* the ext_send_msg texts :294, :209, :216, :274 */
       KG_FAX_ROW_SENT = 16, KG_FAX_PHASING_REJECTED = 32, KG_FAX_MEDIAN = 64 };                           /* :404, :240-243, :238 */
typedef struct kg_fax_rec {                /* one completed line, as it stands behind DecodeFaxLine (:437) */
    int32_t blk, off;                      /* the block of the push and i of :431, counted from behind the skip, at which it completed */
    int32_t type, typecount, imageline, phasingLinesLeft, skip;
    int32_t phasing_pos;                   /* FaxPhasingLinePosition of this line (:227), or -1 */
    int32_t flags;                         /* KG_FAX_* */
    int32_t phasingSkipData, ten_pct, ninety_pct;          /* under KG_FAX_MEDIAN: what :239 prints */
} kg_fax_rec;
typedef struct kg_fax_info {               /* FaxDecoder.h:72-137, what the port keeps of it; fax_t's capture and shift (fax.cpp:20-29) */
    double nom, frac, frac_prev, ratio, fi, lineIncrFrac, lineIncrAcc, lineBlend, carrier, deviation;
    int32_t lpm, imagewidth, bandwidth, include_headers, use_phasing, autostop, autostopped, debug, skip_header_detection, spl;
    int32_t skip, samp_idx, lasttype, typecount, imageline, phasingLinesLeft, phasingSkipData, have_phasing, fir_current, started;
    float Iprev, Qprev;
    float fir[2][17];                      /* firfilter::buffer of the I and the Q filter, in the reference's circular layout */
    int32_t phasingPos[40];
    float shift; int32_t pad;
} kg_fax_info;
/* nconn FaxDecoder objects (FaxDecoder.cpp:51), each zeroed as the static array is; 1 .. 256 */
int kg_fax_create(kg_ctx *ctx, int nconn, kg_fax **out);
/* ~FaxDecoder (FaxDecoder.h:53); drains the context's stream first */
void kg_fax_destroy(kg_fax *q);
/* `SET fax_start` (fax.cpp:128-156): Configure (FaxDecoder.cpp:467-515) with reset, every parameter of it; nom_rate is snd_rate, srate
 * what ext_update_get_sample_rateHz answers now (:92-97).  Iprev, Qprev, m_lineBlend, m_skip and m_SamplesPerSec_frac_prev are carried
 * over, as the reference carries them.  One small launch. */
int kg_fax_start(kg_fax *q, int conn, int lpm, int imagewidth, int carrier, int deviation, int bandwidth, int include_headers, int phasing, int autostop, int debug,
                 double nom_rate, double srate);
/* `SET fax_shift=%f` (fax.cpp:159-165): the next pushed block of a started connection takes it (FaxDecoder.cpp:416) */
int kg_fax_set_shift(kg_fax *q, int conn, float shift);
/* `SET fax_stop` (fax.cpp:167-171, fax_close :94-107): no more samples are taken, the pending shift is dropped; the decoder stays */
int kg_fax_stop(kg_fax *q, int conn);
/* The least max_lines a push of nblk[i] blocks of connection conns[i] needs (FaxDecoder.cpp:426-441: a block gives at most 1026 picks
 * at a rate ratio of 1/2) and the widest imagewidth among the started ones.  Either may be NULL. */
int kg_fax_max_lines(kg_fax *q, const int32_t *conns, int nconn, const int32_t *nblk, int32_t *max_lines, int32_t *max_width);
/* ProcessSamples (FaxDecoder.cpp:410-447) as fax_task calls it (fax.cpp:85-88) for nblk[i] blocks (0 .. 256) of 512 samples of connection
 * conns[i] (each at most once), on HOST arrays: block b of entry i is at s16 + i*stride + 512*b.  srate[i] is what
 * ext_update_get_sample_rateHz answers for every line that completes in this push (:94).  A connection that is not started takes
 * nothing and counts zeros.  Outputs as laid out above; row_stride >= imagewidth + 1.  ONE kernel launch.  Synchronises.  (The push on
 * device-resident audio, enqueue only, is the receiver bank's: kg_rxbank_fax_* below.) */
int kg_fax_push(kg_fax *q, const int32_t *conns, int nconn, const int32_t *nblk, const int16_t *s16, size_t stride, const double *srate, uint8_t *rows,
                size_t row_stride, kg_fax_rec *recs, int max_lines, int32_t *counts);
/* Connection conn's whole object (FaxDecoder.h:72-137), for tests: the scalars, m_samples and m_demod_data, the previous image line
 * (zeros while m_imageline is 0) and m_outImage, KG_FAX_MAX_SPL entries each (any may be NULL).  Synchronises. */
int kg_fax_state(kg_fax *q, int conn, kg_fax_info *info, int16_t *samples, uint8_t *demod, uint8_t *prev, uint8_t *out);

/* ---- The CW decoder extension (extensions/CW_decoder/uhsdr_cw_decoder.cpp, cw_decoder.cpp): Morse code from the 16-bit mono audio a
 * sound block ends as, taken by the real-samples task tap.  Per block of 88 samples a Goertzel magnitude at the passband offset; per
 * magnitude a threshold (fixed or automatic), a ring of mark / space durations, the training of the dot, dash and space averages, the
 * recognition of characters with two corrective actions, the PARIS speed.  Every event is an exact function of the samples and of
 * now_sec: csrc/kg_cw.h is the one definition for device and host, in the reference's operand types, and cites the reference lines item
 * by item.
 *
 * The SCHEDULE depends on the samples, so the whole cw_decoder_t of a connection lives on the device and a push's outputs carry counts
 * the DEVICE writes: for entry i of the list, with max_events the capacity the caller chose (kg_cw_max_events gives the least one),
 *   counts[4*i]      events;  counts[4*i + 1]  Goertzel blocks completed;  counts[4*i + 2]  1 if the capacity was exceeded (never, by the bound)
 *   evs + i*max_events + k                    event k (kg_cw_ev)
 * TIME IS AN INPUT: the reference reads timer_sec() for `cw_wpm` (at most once per 4 s, :983-987) and for err_timeout (:1277, :1289); a
 * push carries now_sec[i], which holds for every block of entry i.  No host clock is read.
 * Defined here where the reference leaves it open (csrc/kg_cw.h has each): `static int slowdown` (:519) is per connection; the float to
 * uint8_t / int16_t conversions of :606 and :1007 are x86-64 gcc's; data[data_len - 1] with data_len 0 (:862, :874) reads sig_timer.
 * Refused with nothing changed: training_interval outside 1 .. 255, wpm negative, a pboff whose Goertzel bin leaves 0 .. 44 or before the
 * first start, a nominal rate outside 88 .. 1e6 Hz, a sample rate that is not finite, not positive or outside half to twice the nominal.
 * Not ported: the test-file player, cw_task's sequence numbers, the printfs. */
typedef struct kg_cw kg_cw;
#define KG_CW_BLK 512                                      /* FASTFIR_OUTBUF_SIZE, cw_decoder.cpp:101 */
#define KG_CW_GBLK 88                                      /* CW_DECODER_BLOCKSIZE_DEFAULT, uhsdr_cw_decoder.h:23 */
#define KG_CW_EVENTS_PER_GBLK 7                            /* csrc/kg_cw.h derives it */
enum { KG_CW_CHARS = 0, KG_CW_WPM = 1, KG_CW_TRAIN = 2, KG_CW_PLOT = 3 };  /* cw_chars :961, cw_wpm :985, cw_train :672 :1278 :1292, cw_plot :525 */
typedef struct kg_cw_ev {                  /* one message of ext_send_msg / ext_send_msg_encoded */
    int32_t blk;                           /* the sound block of the push in which the Goertzel block ended */
    int32_t gblk;                          /* the Goertzel block among those that ended in that sound block */
    int32_t kind;                          /* KG_CW_* */
    int32_t a, b, c;                       /* CHARS a: the character, the prosign index 0..11 (<aa> <ar> <as> <bk> <bt> <cl> <ct> <hh> <kn> <nj> <sk> <sn>),
                                              0xff for [err], or ' ';  WPM a: the speed;  TRAIN a: the value, negative for the error count;
                                              PLOT a, c: the bits of the two floats of `%.2f`, b: the flag */
} kg_cw_ev;
typedef struct kg_cw_info {                /* cw_decoder_t (:106-174), what the port keeps of it; a sigbuf_t is bit 0 state, bits 1..31 time */
    int32_t process_samples; uint32_t wpm_update; int32_t wsc, err_cnt, err_timeout; float sampling_freq; int32_t speed, isAutoThreshold;
    uint32_t weight_linear, threshold_linear; int32_t blocksize;
    int32_t g_a; float g_b, g_sin, g_cos, g_r;             /* Goertzel (:71-79); b0..b2 are zero between blocks */
    int32_t sig_lastrx, sig_incount, sig_outcount, sig_timer;
    int32_t data_len; uint32_t code; int32_t state, initialized, dash, wspace, timeout, track;
    float pulse_avg, dot_avg, dash_avg, symspace_avg, cwspace_avg; int32_t w_space;
    int32_t timer_stepsize, cur_time, cur_outcount, last_outcount;
    float CW_env, CW_mag, CW_noise, old_siglevel, speed_wpm_avg;
    int32_t prevstate, noisecancel_change, sample_counter, startpos, progress, initializing, processed, training_interval;
    int32_t snd_rate, slowdown, started, pad0, pad1;       /* snd_rate (:59), the static of :519, the task tap (cw_decoder.cpp:149) */
    uint32_t sig[256];
    uint32_t data[40];
    float raw[88];                         /* raw_signal_buffer (:128) */
} kg_cw_info;
/* nconn cw_decoder_t objects (:176), each zeroed as the static array is; 1 .. 256 */
int kg_cw_create(kg_ctx *ctx, int nconn, kg_cw **out);
/* nothing in the reference frees them (:176 is static); drains the context's stream first */
void kg_cw_destroy(kg_cw *q);
/* `SET cw_start=%d` and `SET cw_train=%d` (cw_decoder.cpp:135-167): CwDecode_Init(rx_chan, 0, training_interval) (:345-392), a memset with
 * defaults -- the thresholds, the Goertzel and process_samples fall back to 0 until they are sent again -- and the task tap
 * (cw_decoder.cpp:149).  nom_rate is snd_rate (:59), srate what ext_update_get_sample_rateHz answers now (:356).  One small launch. */
int kg_cw_start(kg_cw *q, int conn, int training_interval, double nom_rate, double srate);
/* `SET cw_wpm=%d,%d` (cw_decoder.cpp:186-190): CwDecode_wpm (:628-633), CwDecode_Init with the fixed-WPM branch (:362-385) for wpm != 0; the
 * rates are those of the last kg_cw_start.  Its `EXT cw_train=0` (:385) is implied by the call. */
int kg_cw_set_wpm(kg_cw *q, int conn, int wpm, int training_interval);
/* `SET cw_pboff=%d` (cw_decoder.cpp:179-183): CwDecode_pboff with AudioFilter_CalcGoertzel (:296-305, :394-402); samples are taken from here on */
int kg_cw_set_pboff(kg_cw *q, int conn, uint32_t pboff);
/* `SET cw_wsc=%d` (cw_decoder.cpp:193-197): CwDecode_wsc (:1020-1024) */
int kg_cw_set_wsc(kg_cw *q, int conn, int wsc);
/* `SET cw_auto_thresh=%d` (cw_decoder.cpp:200-204): CwDecode_threshold type 0 (:1030-1036) */
int kg_cw_set_auto_threshold(kg_cw *q, int conn, int on);
/* `SET cw_threshold=%d` (cw_decoder.cpp:207-211): CwDecode_threshold type 1 (:1038) */
int kg_cw_set_threshold(kg_cw *q, int conn, int threshold);
/* `SET cw_stop` (cw_decoder.cpp:155-160, cw_close :107-119): no more samples are taken; the decoder stays */
int kg_cw_stop(kg_cw *q, int conn);
/* The least max_events of a push of nblk sound blocks (0 .. 256): KG_CW_EVENTS_PER_GBLK for each of the (512 nblk + 87) / 88 Goertzel
 * blocks it can complete (:620-623); -1 outside that range */
int kg_cw_max_events(int nblk);
/* CwDecode_RxProcessor (:609-625) as cw_task calls it (cw_decoder.cpp:101) for nblk[i] blocks (0 .. 256) of 512 samples of connection
 * conns[i] (each at most once), on HOST arrays: block b of entry i is at s16 + i*stride + 512*b.  now_sec[i] is what timer_sec() answers
 * during entry i (:983, :1277, :1289).  A connection that is not started, or has had no pboff since its start (:613), takes nothing and
 * counts zeros.  Outputs as laid out above.  ONE kernel launch.  Synchronises.  (The push on device-resident audio, enqueue only, is the
 * receiver bank's: kg_rxbank_cw_* below.) */
int kg_cw_push(kg_cw *q, const int32_t *conns, int nconn, const int32_t *nblk, const int16_t *s16, size_t stride, const uint32_t *now_sec, kg_cw_ev *evs,
               int max_events, int32_t *counts);
/* Connection conn's whole object (:106-174), for tests: the scalars, the ring and data[].  Synchronises. */
int kg_cw_state(kg_cw *q, int conn, kg_cw_info *info);

/* ---- The WSPR extension, stage 1 (extensions/wspr/wspr_main.cpp, wspr.cpp): from the IQ tap (receive_iq_samps: CFastFIR's output of
 * every sound block) to the candidate list.  Capture with drop-sample decimation to 375 Hz into two ping-pong halves synchronised to the
 * even minute (wspr_data, wspr_main.cpp:595-788); per group of four half-symbol steps the windowed 512-point transforms, pwr_samp,
 * pwr_sampavg, savg and the display row of 412 bytes (WSPR_FFT, :117-240, renormalize, wspr.cpp:214-253); at the end of a cycle pass 0
 * of wspr_decode: the peak list (wspr.cpp:555-628) and the coarse search over frequency, time and drift (wspr.cpp:658-714).
 * csrc/kg_wspr.h is the one definition for device and host, in the reference's operand types, and cites the reference item by item.
 * Not in this stage: sync_and_demodulate and everything behind it (the decoders, the hash table, subtraction, later passes),
 * abort_decode, autorun / IWBP, uploads, the test-file player.  i_data / q_data of both halves stay on the device for them.
 *
 * The SCHEDULE depends on no sample: the host walks a push block by block and the kernels get a table; the status changes
 * (wspr_status, :96-114) come out as event records.  TIME IS AN INPUT: every block of a push carries the minute and second that
 * utc_hour_min_sec (:629) would have answered for its callback.  No host clock is read.
 * What passes through the transform (pwr_samp, pwr_sampavg, the rows) is held to a bound, everything from the planes on -- peaks and
 * candidates -- is an exact function of them.  The outputs carry counts the DEVICE writes: for entry i of the list
 *   counts[4*i]  rows written;  counts[4*i + 1]  1 if a cycle ended;  counts[4*i + 2]  its peaks;  cycles[i]  the cycle end (due 0: none)
 * Defined here where the reference leaves it open: the decoder of this stage takes no time (a cycle end's events are DECODING, PEAKS,
 * then status_resume); a row byte whose y is NaN (silence) is 0 and such a cycle has no peaks; ties in snr0 keep frequency order; memory
 * handed out is zeros.  Refused with nothing changed: snd_rate below 375 or not finite, a type other than 2 / 15, a minute or second
 * outside 0 .. 59, a push before kg_wspr_init (KG_ERR_STATE), a push in which one connection completes two cycles. */
typedef struct kg_wspr kg_wspr;
#define KG_WSPR_NBINS 411                                  /* nbins_411, wspr_main.cpp:1155 */
#define KG_WSPR_NFFT 512                                   /* NFFT, wspr.h:160 */
#define KG_WSPR_NT 348                                     /* FPG*GROUPS, wspr.h:225 */
#define KG_WSPR_TPOINTS 45000                              /* wspr.h:147 */
#define KG_WSPR_MAX_NPK 12                                 /* wspr.h:183 */
#define KG_WSPR_ROW_STRIDE 416                             /* a row's 412 bytes (WSPR_DATA, :238) start at multiples of this */
enum { KG_WSPR_IDLE = 1, KG_WSPR_SYNC = 2, KG_WSPR_RUNNING = 3, KG_WSPR_DECODING = 4 };            /* wspr_main.cpp:49-53 */
enum { KG_WSPR_EV_STATUS = 0, KG_WSPR_EV_PEAKS = 1 };
typedef struct kg_wspr_row {               /* one ext_send_msg_data of :238 */
    int32_t conn, blk, samp;               /* the block of the push and the sample of it at which the group was due */
    int32_t group, half, tsync;            /* FFTtask_group, fft_ping_pong, byte 0 */
    int64_t off;                           /* of the row in the byte array */
} kg_wspr_row;
typedef struct kg_wspr_ev {                /* STATUS: a the status, b the resume (0: NONE), `EXT WSPR_STATUS=` (:106); PEAKS: a the half, `WSPR_PEAKS` (:299) */
    int32_t conn, blk, samp, kind, a, b;   /* blk -1: sent by a command since the last push */
} kg_wspr_ev;
typedef struct kg_wspr_pk { int32_t bin0; float freq0, snr0; int32_t pad; } kg_wspr_pk;            /* frequency order, wspr.cpp:612-624 */
typedef struct kg_wspr_cand { float freq0; int32_t shift0; float drift0, sync0; int32_t freq_idx, bin0; } kg_wspr_cand;    /* SNR order, wspr.cpp:627, :701-705 */
typedef struct kg_wspr_cycle { int32_t due, half, npk, pad; kg_wspr_pk pk[KG_WSPR_MAX_NPK]; kg_wspr_cand cand[KG_WSPR_MAX_NPK]; } kg_wspr_cycle;
typedef struct kg_wspr_info {              /* wspr_t (wspr.h:239-312), what this stage keeps of it */
    int32_t inited, capture, reset, tsync, ping_pong, fft_ping_pong, decode_ping_pong, decim, didx, group;
    int32_t status, status_resume, last_sec, abort_decode, wspr_type, more_candidates, int_decimate, cycles;
    double snd_rate;
} kg_wspr_info;
/* nconn wspr_t / wspr_buf_t pairs (wspr.h:223-312), zeroed as wspr_main does (:1163), and the window of :1186-1188; 1 .. 256 */
int kg_wspr_create(kg_ctx *ctx, int nconn, kg_wspr **out);
/* wspr_close (:802-824) frees nothing of them; drains the context's stream first */
void kg_wspr_destroy(kg_wspr *q);
/* `SET ext_server_init` (:834-838): status IDLE; int_decimate = (int) (snd_rate / 375.0) as wspr_main has it (:1193), per connection */
int kg_wspr_init(kg_wspr *q, int conn, double snd_rate);
/* `SET capture=%d` (:880-900): on, a reset at the next callback and status SYNC; off, wspr_close with wspr_reset (:790-800) */
int kg_wspr_set_capture(kg_wspr *q, int conn, int capture);
/* wspr_type (wspr.h:255-257, set by wspr_main, :1170): 2 or 15; it selects snr_scaling_factor (wspr.cpp:247) */
int kg_wspr_set_type(kg_wspr *q, int conn, int type);
/* more_candidates (wspr.h:254, read at wspr.cpp:565) */
int kg_wspr_set_more_candidates(kg_wspr *q, int conn, int on);
/* wspr_data (:595-788) for nblk[i] callbacks (0 .. 4096) of ns complex samples (1 .. 131072) of connection conns[i] (each at most once),
 * on HOST arrays: block b of entry i is at iq + 2*(i*iq_stride + ns*b), its time at minute / second[i*time_stride + b].  Rows go to
 * rows + row_map[r].off (412 bytes each), in the order the reference sends them; events in order per entry, entries in list order.
 * ONE kernel launch, and one more when a cycle ends.  Synchronises. */
int kg_wspr_push(kg_wspr *q, const int32_t *conns, int nconn, const int32_t *nblk, int ns, const float *iq, size_t iq_stride, const int32_t *minute,
                 const int32_t *second, size_t time_stride, uint8_t *rows, size_t rows_cap, kg_wspr_row *row_map, int max_rows, int32_t *nrows, kg_wspr_ev *evs,
                 int max_events, int32_t *nevents, kg_wspr_cycle *cycles, int32_t *counts);
/* The schedule of kg_wspr_push (:595-788) walked on copies: how many ops (copy runs, clears, groups), rows, events and cycle ends the
 * push will emit (any may be NULL).  Changes nothing, touches no device. */
int kg_wspr_plan(kg_wspr *q, const int32_t *conns, int nconn, const int32_t *nblk, int ns, const int32_t *minute, const int32_t *second, size_t time_stride,
                 int32_t *nops, int32_t *nrows, int32_t *nevents, int32_t *ncycles);
/* Connection conn's object (wspr.h:223-312), for tests and for a host that saves it: the scalars, pwr_sampavg [2][512], pwr_samp
 * [2][512][348] and i_data then q_data [2][2][45000], each as the reference lays it out (any may be NULL).  Synchronises. */
int kg_wspr_state(kg_wspr *q, int conn, kg_wspr_info *info, float *pwr_sampavg, float *pwr_samp, float *iq_data);
/* For a host that resumes, and for tests: pwr_samp [512][348] and pwr_sampavg [512] placed into a half, then the cycle end on it (pass 0
 * of wspr_decode, wspr.cpp:555-714) under the connection's type and more_candidates.  One launch.  Synchronises. */
int kg_wspr_load(kg_wspr *q, int conn, int half, const float *pwr_samp, const float *pwr_sampavg, kg_wspr_cycle *cycle);
/* Stage 2 of the WSPR extension -- fine sync, soft symbols and the Fano decoder on the candidates a connection holds -- is declared in a
 * header of its own, in this directory. */
#include "kiwigpu_wspr_dec.h"
#include "kiwigpu_ft8.h"

/* Diagnostics: re-runs the 4096-point stage of the forward FFT of `block` in a
 * stamped build of the kernel and returns 4 s_memrealtime readings (100 MHz):
 * start, inputs + twiddles loaded, transform done, results stored. */
int kg_acq_debug_fft_stamps(kg_acq *acq, int block, unsigned long long *stamps, int n);
/* Diagnostics: one Correlate() launch in a stamped build; stamps[0..3] = kernel
 * start/end (s_memtime cycles, s_memrealtime 100 MHz) of one workgroup, then 16
 * s_memtime readings per 4096-point work item (24 items) from stamps[16]; from stamps[512],
 * four values per workgroup b: start, end (s_memrealtime), XCC id register, cells done.
 * n >= 4608. */
int kg_acq_debug_corr_stamps(kg_acq *acq, int nblocks, const int *sats, int nsats,
                             unsigned long long *stamps, int n);

/* ------------------------------------------------------------------------ */
/* A bank of virtual receivers stepped with ONE call (round 5; BASELINE           */
/* configs[3]).  In the reference every connection runs a waterfall and a sound   */
/* coroutine over what the data pump hands them: data_pump()                      */
/* (rx/data_pump.cpp:292-341), the c2s_sound() loop (rx/rx_sound.cpp:333-601:     */
/* in_samps -> CFastFIR -> S-meter / AGC / demod -> compression) and               */
/* c2s_waterfall() -> sample_wf() -> compute_frame() -> wf_pkt_t                    */
/* (rx/rx_waterfall.cpp:930-1170).  A bank is nrx such connections fed from one     */
/* block of ADC samples per step; kg_rxbank_step() enqueues everything a step        */
/* needs -- both DDCs, frames, packets, unpack, CFastFIR, S-meter / CAgc, ADPCM --   */
/* on the bank's own streams, with ONE host-to-device transfer (the small tables     */
/* of all stages) per step.  The per-seam objects are the bank's and are configured  */
/* with their own entry points above (tables, maps, frequencies, filters, AGC).      */
/* ------------------------------------------------------------------------ */
typedef struct kg_rxbank kg_rxbank;

/* nrx receivers on `device`, adc_samples_per_step int16 ADC samples per step, audio DDCs of rx_mode (KG_RXDDC_*). */
int kg_rxbank_create(int device, int nrx, size_t adc_samples_per_step, int rx_mode, kg_rxbank **out);
void kg_rxbank_destroy(kg_rxbank *bank);
/* The owned objects, channel k = receiver k (never destroy them; reconfigure only between steps -- the setters of the
 * objects synchronise their own stream). */
kg_ctx *kg_rxbank_ctx(kg_rxbank *bank);       /* the waterfall chain's context: kg_dev_download etc. */
kg_ddc *kg_rxbank_ddc(kg_rxbank *bank);       /* do NOT call kg_ddc_set_wf on it: kg_rxbank_set_wf */
kg_wf *kg_rxbank_wf(kg_rxbank *bank);         /* kg_wf_set_tables, kg_wf_set_channel */
kg_rxddc *kg_rxbank_rxddc(kg_rxbank *bank);   /* kg_rxddc_set_freq */
kg_fir *kg_rxbank_fir(kg_rxbank *bank);       /* kg_fir_setup */
kg_post *kg_rxbank_post(kg_rxbank *bank);     /* kg_post_set_agc / _set_smeter / _set_mode / _reset */
kg_adpcm *kg_rxbank_adpcm(kg_rxbank *bank);
/* The noise blankers (NB_STD, NB_WILD) of the bank's receivers: m_NoiseProc_snd[] (kg_nb; the waterfall's m_NoiseProc_wf[] are
 * kg_rxbank_wf's) and nb_Wild[] (kg_rxbank_post's kg_post_nbw_*).
 * The commands keep snd_t's and wf_inst_t's NB state per receiver, with the reference's side effects on both:
 *   kg_rxbank_set_nb_algo    `SET nb algo=` (rx_sound_cmd.cpp:454-462): the algo; both the audio and the waterfall enables cleared.
 *   kg_rxbank_nbw_select     `SET nb algo=2`: the same with algo = KG_NB_WILD (kg_rxbank_set_nb_algo keeps refusing the value); no
 *                            blanker state touched.
 *   kg_rxbank_set_nb_enable  `SET nb type= en=` (:477-483): both enables of that type.
 *   kg_rxbank_set_nb_param   `SET nb type= param= pval=` (:485-501): the audio value stored; under NB_STD or for NB_CLICK also the
 *                            waterfall's, with its change pending; NB_BLANKER under NB_STD: SetupBlanker("SND", frate, ...) at once;
 *                            NB_BLANKER under NB_WILD: nb_Wild_init from the whole stored vector (kg_post_nbw_init: state and history
 *                            zeroed on every message), nothing stored on the waterfall side.
 *   kg_rxbank_set_nb_gate    kiwiclient's `SET nb= th=` (:660-672): gate, threshold and the audio enable only; SetupBlanker when nb != 0,
 *                            whatever the algo; never nb_Wild_init.
 * Under NB_WILD the audio enable of NB_BLANKER (kg_rxbank_set_nb_enable, kg_rxbank_set_nb_gate) is the Wild stage's switch
 * (kg_post_set_nbw): the stage runs inside the step's kg_post pass, behind de-emphasis, and delays the receiver's audio by order + PL
 * samples; the step's NB_STD audio blanker does not run; the waterfall side keeps the rules below.  Selecting any algo,
 * kg_rxbank_join and kg_post_reset switch the stage off.
 * A step runs the audio blanker in place on the unpacked records (kg_rxbank_bufs.rx_in: what CFastFIR was fed) of every active
 * receiver with enable[NB_BLANKER] under NB_STD (rx_sound.cpp:593-598).  Before a receiver's next frame, with both waterfall
 * enables (NB_BLANKER, NB_WF) on, a pending change sets up its waterfall blanker (kg_wf_nb_setup); its frames are then blanked
 * (rx_waterfall.cpp:1087-1099).  A zoom change through kg_rxbank_set_wf (decimation) or kg_rxbank_set_wf_pkt (zoom) makes the change
 * pending when both enables are on (:460).  kg_rxbank_join clears the receiver's NB command state on both sides (algo NB_OFF,
 * enables, params, pending changes, nb_setup) and keeps the blankers' states.
 * Refused at the command, nothing changed: KG_NB_WILD in kg_rxbank_set_nb_algo (KG_ERR_INVALID: kg_rxbank_nbw_select) or a value that
 * is no nb_algo_e (KG_ERR_INVALID); a type outside 0..3 or a
 * param outside 0..7 (KG_ERR_INVALID); enabling KG_NB_CLICK (KG_ERR_INVALID: test pulses are not implemented); enabling
 * KG_NB_BLANKER under KG_NB_STD before the audio blanker was set up (KG_ERR_STATE); a value that kg_nb_setup refuses at frate (audio)
 * or at 8192 (the waterfall's); under KG_NB_WILD, enabling KG_NB_BLANKER on a vector NB_Wild.cpp cannot run on (KG_ERR_STATE) and a
 * parameter that makes the vector such a one while the stage is on (KG_ERR_INVALID): see kg_post_nbw_init. */
kg_nb *kg_rxbank_nb(kg_rxbank *bank);
int kg_rxbank_set_nb_algo(kg_rxbank *bank, int rx, int algo);
int kg_rxbank_nbw_select(kg_rxbank *bank, int rx);
int kg_rxbank_set_nb_enable(kg_rxbank *bank, int rx, int type, int en);
int kg_rxbank_set_nb_param(kg_rxbank *bank, int rx, int type, int param, float pval, float frate);
int kg_rxbank_set_nb_gate(kg_rxbank *bank, int rx, int nb, int th, float frate);
/* The command state of receiver rx: ints[14] = algo, snd enable[4], wf enable[4], wf nb_param_change[4], wf nb_setup; flts[64] =
 * snd nb_param[4][8], wf nb_param[4][8] (either may be NULL). */
int kg_rxbank_nb_cmd_state(kg_rxbank *bank, int rx, int32_t *ints, float *flts);
/* The audio spectrum rows of the bank's receivers (see kg_snd_spec_rows_dev).
 *   kg_rxbank_set_spec   `SET spc_=%d` (rx_sound_cmd.cpp:332-339): n outside 0..2 becomes 0; only 2 (SPEC_SND_AF) switches the
 *                        receiver's rows on.  kg_rxbank_join clears it.
 *   kg_rxbank_null_fir   the bank's second kg_fir, m_chan_null_FIR[] (rx_sound.cpp:151): the host designs it together with the
 *                        passband filter (kg_fir_setup on both, rx_sound_cmd.cpp:274-275).  kg_rxbank_join resets the receiver's
 *                        channel in it.  A receiver that reaches channel-null SAM without a filter there fails the step.
 * A step's one CFastFIR launch gives the passband rows.  Behind a sound block's kg_post pass, every receiver that ran it in
 * KG_POST_SAM with mparam & 3 feeds that block's 512 nulled AGC samples (bufs.agc) to the channel-null filter without an output
 * buffer, whether its rows are on or not (rx_sound.cpp:804).  Which blocks give a row is the reference's rule, kept per receiver
 * on the host as a mirror of s->specAF_instance / s->isChanNull (rx_sound_cmd.cpp:227-228, rx_sound.cpp:802-803): cleared by every
 * kg_post_set_mode and kg_post_set_sam_mparam on the bank's kg_post, set behind a processed block to mode == SAM && (mparam & 3).
 * A passband block gives a row (x 1e6) only while the mirror says PASSBAND at that block -- the first block after entering
 * channel-null SAM still does; the channel-null filter gives one (x 0.0004) per 1024-sample fill of its own.
 *   kg_rxbank_spec_map   the rows of the last step, row r at d_rows + r*row_stride: receiver, KG_SPEC_* instance and sound block of
 *                        the step (arrays of kg_rxbank_spec_max() entries, any may be NULL), per receiver in the reference's
 *                        emission order -- a block's passband row, then the channel-null row completed by feeding that block.
 *                        Returns the number of rows.  The host sends each behind kg_snd_spec_due.
 *   kg_rxbank_spec_rows  the device buffer (valid until kg_rxbank_destroy; read behind kg_rxbank_sync).
 * A step in which no receiver has its rows on and none is in channel-null SAM enqueues what it enqueued without any of this. */
int kg_rxbank_set_spec(kg_rxbank *bank, int rx, int n);
kg_fir *kg_rxbank_null_fir(kg_rxbank *bank);
int kg_rxbank_spec_max(kg_rxbank *bank);
int kg_rxbank_spec_map(kg_rxbank *bank, int32_t *rx_of_row, int32_t *inst_of_row, int32_t *blk_of_row);
int kg_rxbank_spec_rows(kg_rxbank *bank, void **d_rows, size_t *row_stride);

/* The FFT extension of the bank's receivers (kg_fftext above; extensions/FFT/FFT.cpp).  The first of these calls makes the bank's
 * kg_fftext object and two buffers (the step's filtered spectra of both filters, the rows) and drains the bank's streams; a bank that
 * was never told holds nothing for the extension and enqueues exactly what it enqueued without it.
 *   kg_rxbank_fftext_set_rate   what ext_update_get_sample_rateHz answers (the bank's audio rate as the host knows it, a double)
 *   kg_rxbank_fftext_set_run    `SET run=%d`: snd->isSAM and snd->mode == MODE_QAM are read from the receiver's kg_post mode AT THE
 *                               COMMAND, as the reference reads them (a later `SET mod=` does not move the instance or the boost)
 *   kg_rxbank_fftext_set_itime  `SET itime=%lf`;   kg_rxbank_fftext_clear  `SET clear`
 * While a receiver's function is on, its passband filter's spectrum of every completed block is stored, and in channel-null SAM the
 * second filter's too; the extension runs once per step, in one launch over the step's blocks of all such receivers, behind both
 * filters.  spec chosen in a SAM-family mode listens to the second filter, which is fed in channel-null SAM only: in plain SAM the
 * function shows nothing, as in the reference.  kg_rxbank_join and kg_rxbank_leave put the receiver's extension state back to a new
 * connection's (function off, period 0, sums zero).  A step whose blocks the extension refuses (an integ block before any period was
 * set: KG_ERR_STATE) is refused as a whole, nothing enqueued.
 *   kg_rxbank_fftext       the object (NULL until one of the calls above): kg_fftext_due per row, kg_fftext_state
 *   kg_rxbank_fftext_map   the rows of the last step, row r at d_rows + r*row_stride: receiver, sound block of the step and bin (arrays
 *                          of kg_rxbank_fftext_max() entries, any may be NULL), per receiver in block order.  Returns the number of rows.
 *   kg_rxbank_fftext_rows  the device buffer (NULL until the extension was named; read behind kg_rxbank_sync). */
int kg_rxbank_fftext_set_rate(kg_rxbank *bank, double sample_rate);
int kg_rxbank_fftext_set_run(kg_rxbank *bank, int rx, int run);
int kg_rxbank_fftext_set_itime(kg_rxbank *bank, int rx, double itime);
int kg_rxbank_fftext_clear(kg_rxbank *bank, int rx);
kg_fftext *kg_rxbank_fftext(kg_rxbank *bank);
int kg_rxbank_fftext_max(kg_rxbank *bank);
int kg_rxbank_fftext_map(kg_rxbank *bank, int32_t *rx_of_row, int32_t *blk_of_row, int32_t *bin_of_row);
int kg_rxbank_fftext_rows(kg_rxbank *bank, uint8_t **d_rows, size_t *row_stride);

/* The IQ display extension of the bank's receivers (kg_iqd above; extensions/IQ_display/iq_display.cpp).  The first of these calls makes
 * the bank's kg_iqd object and two buffers (the rows, the status records) and drains the bank's streams; a bank that was never told
 * holds nothing for the extension (but room for its table in the step's arena slots, whose size is fixed at kg_rxbank_create) and
 * enqueues exactly what it enqueued without it.  The commands are kg_iqd's, per receiver:
 * kg_rxbank_iqd_init (`SET ext_server_init`), kg_rxbank_iqd_set_run (`SET run=%d` with what ext_update_get_sample_rateHz answers) and
 * the seven of process_msg.  While a receiver has run on and is not in KG_POST_NBFM in a step (receive_iq_pre_agc is NULL while isNBFM,
 * rx_sound.cpp:492), the CFastFIR output of its sound blocks of that step feeds the extension as instance 0: ONE launch per step over
 * all such receivers, on the tail stream behind the filter.  kg_rxbank_join and kg_rxbank_leave give the receiver a fresh object, run
 * off.  A step the extension refuses (more rows than the map holds: 512 per receiver and sound block, 2^18 at most) is refused as a
 * whole, nothing enqueued.
 *   kg_rxbank_iqd         the object (NULL until one of the calls above): kg_iqd_state
 *   kg_rxbank_iqd_map     the rows of the last step (kg_iqd_row: ch the receiver, blk the sound block of the step, off from d_rows);
 *                         row_map may be NULL.  Returns the number of rows.
 *   kg_rxbank_iqd_rows    the device buffer and its size, (512 B + 16384) * 4 bytes per receiver for a step of up to B sound blocks
 *                         (NULL until the extension was named; read behind kg_rxbank_sync)
 *   kg_rxbank_iqd_status  the status records of the last step, one per fed (receiver, sound block) in the order of the call: the
 *                         device buffer, and on the host whose record k is and whether the reference sends it (arrays of nrx x the
 *                         step's largest block count; any may be NULL).  Returns the number of records. */
int kg_rxbank_iqd_init(kg_rxbank *bank, int rx);
int kg_rxbank_iqd_set_run(kg_rxbank *bank, int rx, int run, double rate);
int kg_rxbank_iqd_set_gain(kg_rxbank *bank, int rx, int gain);
int kg_rxbank_iqd_set_points(kg_rxbank *bank, int rx, int points);
int kg_rxbank_iqd_set_pll_mode(kg_rxbank *bank, int rx, int pll_mode, int arg);
int kg_rxbank_iqd_set_pll_bandwidth(kg_rxbank *bank, int rx, float bandwidth);
int kg_rxbank_iqd_set_draw(kg_rxbank *bank, int rx, int draw);
int kg_rxbank_iqd_set_display_mode(kg_rxbank *bank, int rx, int display_mode);
int kg_rxbank_iqd_clear(kg_rxbank *bank, int rx);
kg_iqd *kg_rxbank_iqd(kg_rxbank *bank);
int kg_rxbank_iqd_map(kg_rxbank *bank, kg_iqd_row *row_map, int max_rows);
int kg_rxbank_iqd_rows(kg_rxbank *bank, uint8_t **d_rows, size_t *rows_cap);
int kg_rxbank_iqd_status(kg_rxbank *bank, kg_iqd_status **d_status, int32_t *rx_of_blk, int32_t *blk_of_blk, int32_t *sent_of_blk);

/* The Loran-C extension of the bank's receivers (kg_lorc above; extensions/Loran_C/loran_c.cpp).  The first of these calls makes the
 * bank's kg_lorc object and its row buffer, grows the step's arena slots by the size of the extension's table and drains the bank's
 * streams; a bank that was never told holds nothing for the extension and enqueues exactly what it enqueued without it.  While a
 * receiver is started and not in KG_POST_NBFM in a step (receive_iq_pre_agc is NULL while isNBFM, rx_sound.cpp:492), the CFastFIR
 * output of its sound blocks of that step feeds the extension in place: ONE launch per step over all such receivers, on the tail
 * stream behind the filter.  kg_rxbank_join and kg_rxbank_leave give the receiver a fresh object, stopped.  The tap holds ONE callback
 * (ext_users[rx].receive_iq_pre_agc): kg_rxbank_lorc_start on a receiver whose IQ display has run on, and kg_rxbank_iqd_set_run(.., 1,
 * ..) on a receiver with Loran-C started, are refused (KG_ERR_STATE). */
/* `SET ext_server_init` (:218-228) of receiver rx: kg_lorc_init */
int kg_rxbank_lorc_init(kg_rxbank *bank, int rx, double srate, int i_srate);
/* `SET gri%d=%d` (:230-240): kg_lorc_set_gri; a bank also refuses a GRI of fewer than 128 samples (it bounds a step's table by it) */
int kg_rxbank_lorc_set_gri(kg_rxbank *bank, int rx, int ch, int gri);
/* `SET offset%d=%d` (:242-250): kg_lorc_set_offset */
int kg_rxbank_lorc_set_offset(kg_rxbank *bank, int rx, int ch, int offset);
/* `SET gain%d=%d` (:252-260): kg_lorc_set_gain */
int kg_rxbank_lorc_set_gain(kg_rxbank *bank, int rx, int ch, int gain);
/* `SET avg_algo%d=%d` (:262-269): kg_lorc_set_avg_algo */
int kg_rxbank_lorc_set_avg_algo(kg_rxbank *bank, int rx, int ch, int avg_algo);
/* `SET avg_param%d=%lf` (:271-280): kg_lorc_set_avg_param */
int kg_rxbank_lorc_set_avg_param(kg_rxbank *bank, int rx, int ch, double avg_param);
/* `SET start` (:282-292): kg_lorc_start.  A step with a started receiver whose push kg_lorc refuses (a channel without a GRI, EMA
 * below 1, IIR negative or non-finite) is refused as a whole, nothing enqueued. */
int kg_rxbank_lorc_start(kg_rxbank *bank, int rx);
/* `SET stop` (:294-302): kg_lorc_stop */
int kg_rxbank_lorc_stop(kg_rxbank *bank, int rx);
/* the object (NULL until one of the calls above), for kg_lorc_state (:29-52) */
kg_lorc *kg_rxbank_lorc(kg_rxbank *bank);
/* the rows of the last step (ext_send_msg_data, :119-120; kg_lorc_row: conn the receiver, blk the sound block of the step, off from
 * d_rows); row_map may be NULL.  Returns the number of rows. */
int kg_rxbank_lorc_map(kg_rxbank *bank, kg_lorc_row *row_map, int max_rows);
/* the device buffer of the step's rows (e->scope, :50) and its size (NULL until the extension was named; read behind kg_rxbank_sync) */
int kg_rxbank_lorc_rows(kg_rxbank *bank, uint8_t **d_rows, size_t *cap);

/* The FAX extension of the bank's receivers (kg_fax above; extensions/FAX/FaxDecoder.cpp, fax.cpp).  The first of these calls makes the
 * bank's kg_fax object and its output buffers, grows the step's arena slots by the size of the extension's table and drains the
 * bank's streams; a bank that was never told holds nothing for the extension and enqueues exactly what it enqueued without it.  While
 * a receiver is started and the step puts its blocks on the mono list -- the branch in which the reference advances real_wr_pos
 * (rx_sound.cpp:701-703, :1103), so not in KG_POST_IQ, _SAS or _QAM --, the 16-bit audio of its sound blocks of that step feeds the
 * extension in place: ONE launch per step over all such receivers, on the tail stream behind the detectors and ahead of the coders'
 * event.  kg_rxbank_join and kg_rxbank_leave give the receiver a fresh object, not started.  The real-samples tap is another callback
 * than the IQ tap (ext_users[rx].receive_real_tid): FAX runs beside a running IQ display or Loran-C. */
/* `SET fax_start` (fax.cpp:128-156): kg_fax_start; srate stays the receiver's ext_update_get_sample_rateHz (FaxDecoder.cpp:94) until
 * the next start.  A bank also refuses fewer than 1024 samples a line and an imagewidth above 4096 (they bound a step's outputs). */
int kg_rxbank_fax_start(kg_rxbank *bank, int rx, int lpm, int imagewidth, int carrier, int deviation, int bandwidth, int include_headers, int phasing, int autostop,
                        int debug, double nom_rate, double srate);
/* `SET fax_shift=%f` (fax.cpp:159-165): kg_fax_set_shift */
int kg_rxbank_fax_set_shift(kg_rxbank *bank, int rx, float shift);
/* `SET fax_stop` (fax.cpp:167-171): kg_fax_stop */
int kg_rxbank_fax_stop(kg_rxbank *bank, int rx);
/* the object (NULL until one of the calls above), for kg_fax_state (FaxDecoder.h:72-137) */
kg_fax *kg_rxbank_fax(kg_rxbank *bank);
/* The outputs of the last step (FaxDecoder.cpp:404, :437), device memory laid out as kg_fax_push lays its outputs out (NULL until the
 * extension was named; read behind kg_rxbank_sync): entry e is receiver rx_of_entry[e], in receiver order; a record's blk is the sound
 * block of the step.  Any pointer may be NULL.  Returns the number of entries: the receivers the step fed. */
int kg_rxbank_fax_out(kg_rxbank *bank, uint8_t **d_rows, size_t *row_stride, kg_fax_rec **d_recs, int32_t **d_counts, int32_t *max_lines, int32_t *rx_of_entry,
                      int max_entries);

/* The CW decoder extension of the bank's receivers (kg_cw above; extensions/CW_decoder/uhsdr_cw_decoder.cpp, cw_decoder.cpp).  The first
 * of the per-receiver calls makes the bank's kg_cw object and its output buffers, grows the step's arena slots by the size of the
 * extension's table and drains the bank's streams; a bank that was never told holds nothing for the extension and enqueues exactly
 * what it enqueued without it.  A started receiver is fed exactly as FAX is: while the step puts its blocks on the mono list
 * (rx_sound.cpp:701-703, :1103; not KG_POST_IQ, _SAS or _QAM), the 16-bit audio of its sound blocks of that step feeds the extension
 * in place: ONE launch per step over all such receivers, on the tail stream behind FAX's and ahead of the coders' event.
 * kg_rxbank_join and kg_rxbank_leave give the receiver the zeroed object, not started.  The real-samples task tap holds ONE task per
 * receiver (ext_register_receive_real_samps_task, cw_decoder.cpp:149, fax.cpp:150): kg_rxbank_cw_start beside a started FAX and
 * kg_rxbank_fax_start beside a started CW decoder are refused (KG_ERR_STATE); the CW decoder runs beside the IQ display or Loran-C. */
/* `SET cw_start=%d` / `SET cw_train=%d` (cw_decoder.cpp:135-167): kg_cw_start */
int kg_rxbank_cw_start(kg_rxbank *bank, int rx, int training_interval, double nom_rate, double srate);
/* `SET cw_wpm=%d,%d` (cw_decoder.cpp:186-190): kg_cw_set_wpm */
int kg_rxbank_cw_set_wpm(kg_rxbank *bank, int rx, int wpm, int training_interval);
/* `SET cw_pboff=%d` (cw_decoder.cpp:179-183): kg_cw_set_pboff */
int kg_rxbank_cw_set_pboff(kg_rxbank *bank, int rx, uint32_t pboff);
/* `SET cw_wsc=%d` (cw_decoder.cpp:193-197): kg_cw_set_wsc */
int kg_rxbank_cw_set_wsc(kg_rxbank *bank, int rx, int wsc);
/* `SET cw_auto_thresh=%d` (cw_decoder.cpp:200-204): kg_cw_set_auto_threshold */
int kg_rxbank_cw_set_auto_threshold(kg_rxbank *bank, int rx, int on);
/* `SET cw_threshold=%d` (cw_decoder.cpp:207-211): kg_cw_set_threshold */
int kg_rxbank_cw_set_threshold(kg_rxbank *bank, int rx, int threshold);
/* `SET cw_stop` (cw_decoder.cpp:155-160): kg_cw_stop */
int kg_rxbank_cw_stop(kg_rxbank *bank, int rx);
/* what timer_sec() answers (uhsdr_cw_decoder.cpp:983, :1277, :1289) during every later step: it goes into the step's table.  Makes nothing. */
int kg_rxbank_cw_set_now(kg_rxbank *bank, uint32_t now_sec);
/* the object (NULL until one of the per-receiver calls above), for kg_cw_state (uhsdr_cw_decoder.cpp:106-174) */
kg_cw *kg_rxbank_cw(kg_rxbank *bank);
/* The outputs of the last step (uhsdr_cw_decoder.cpp:525, :672, :961, :985), device memory laid out as kg_cw_push lays its outputs out
 * (NULL until the extension was named; read behind kg_rxbank_sync): entry e is receiver rx_of_entry[e], in receiver order; an event's
 * blk is the sound block of the step.  Any pointer may be NULL.  Returns the number of entries: the receivers the step fed. */
int kg_rxbank_cw_out(kg_rxbank *bank, kg_cw_ev **d_evs, int32_t **d_counts, int32_t *max_events, int32_t *rx_of_entry, int max_entries);

/* The WSPR extension of the bank's receivers, stage 1 (kg_wspr above; extensions/wspr/wspr_main.cpp, wspr.cpp).  The first of the
 * per-receiver calls makes the bank's kg_wspr object and its output buffers, grows the step's arena slots by the size of the extension's
 * table and drains the bank's streams; a bank that was never told holds nothing for it.  A refusal at first use leaves the bank as it was.
 * WSPR is the third consumer of the IQ tap (ext_register_receive_iq_samps, wspr_main.cpp:891): while a receiver captures and is not in
 * NBFM, the step's CFastFIR output feeds it in place -- ONE launch per step, and the cycle-end launch behind it when a receiver
 * completes group 85, on the tail stream ahead of the step's end.  The tap holds ONE callback: kg_rxbank_wspr_set_capture(1) beside a
 * running IQ display or a started Loran-C is refused (KG_ERR_STATE), and they are refused beside it.  Join and leave give the receiver
 * a fresh object. */
/* `SET ext_server_init` (wspr_main.cpp:834-838): kg_wspr_init */
int kg_rxbank_wspr_init(kg_rxbank *bank, int rx, double snd_rate);
/* `SET capture=%d` (wspr_main.cpp:880-900): kg_wspr_set_capture; on, it takes the IQ tap */
int kg_rxbank_wspr_set_capture(kg_rxbank *bank, int rx, int capture);
/* wspr_type (wspr.h:255-257): kg_wspr_set_type */
int kg_rxbank_wspr_set_type(kg_rxbank *bank, int rx, int type);
/* more_candidates (wspr.h:254): kg_wspr_set_more_candidates */
int kg_rxbank_wspr_set_more_candidates(kg_rxbank *bank, int rx, int on);
/* what utc_hour_min_sec (wspr_main.cpp:629) answers during every later step: all blocks of a step carry it.  0 .. 59 each */
int kg_rxbank_wspr_set_now(kg_rxbank *bank, int minute, int second);
/* the object (NULL until one of the per-receiver calls above), for kg_wspr_state (wspr.h:223-312) */
kg_wspr *kg_rxbank_wspr(kg_rxbank *bank);
/* The outputs of the last step (wspr_main.cpp:106, :238, :299): the rows' device buffer (row r at row_map[r].off, conn the receiver, blk the
 * sound block of the step), the cycles and counts of every list entry as kg_wspr_push lays them out, device memory valid until the next
 * step; the row map and the events, which are the host's; the receivers of the entries.  Any may be NULL.  Returns the entries. */
int kg_rxbank_wspr_out(kg_rxbank *bank, uint8_t **d_rows, kg_wspr_cycle **d_cycles, int32_t **d_counts, kg_wspr_row *row_map, int max_rows, int32_t *nrows,
                       kg_wspr_ev *evs, int max_events, int32_t *nevents, int32_t *rx_of_entry, int max_entries);
/* CmdSetWFFreq + CmdSetWFDecim + the sampler mode sample_wf() decides on (rx/rx_waterfall.cpp:962-1008):
 *   overlapped == 0   CmdWFReset + the one-shot sampler every step: the non-overlapped frame (:1005-1041); needs
 *                     8192 * decim <= adc_samples_per_step
 *   overlapped == 1   the continuous sampler (CmdWFReset with WF_SAMP_CONTIN, :971-978): every step adds
 *                     adc_samples_per_step / decim outputs (a divisor of 8192) to the receiver's ring and the frame is the
 *                     ring's newest 8192 outputs (CmdGetWFContSamps, :980-991); no frame until the ring holds 8192
 *                     ("fill pipe", :978).  Set kg_wf_chan_cfg.overlapped accordingly (it switches the CIC compensation off).
 * Resets the receiver's sampler.  Synchronises the bank. */
int kg_rxbank_set_wf(kg_rxbank *bank, int rx, uint64_t phase_inc, int decim, int overlapped);
/* Connections come and go one at a time (every c2s_sound() / c2s_waterfall() of the reference is its own loop with its own
 * CFastFIR position and sequence numbers, rx/rx_sound.cpp:264-269, 503-613).  A fresh bank has every receiver active.
 * kg_rxbank_leave: the receiver is skipped by every stage from the next step on.  kg_rxbank_join: its audio DDC, CFastFIR,
 * S-meter / detector, ADPCM state and sound sequence number start from zero and its waterfall sampler waits for
 * kg_rxbank_set_wf; the OTHER receivers are not touched -- from here on this receiver's records per step and the steps on
 * which its 512-sample sound blocks complete are its own (kg_rxbank_audio_map).  Between steps; join drains the bank. */
int kg_rxbank_join(kg_rxbank *bank, int rx);
int kg_rxbank_leave(kg_rxbank *bank, int rx);
int kg_rxbank_is_active(kg_rxbank *bank, int rx);
/* Per receiver after the last step (arrays of nrx entries, any may be NULL): records and CFastFIR outputs (0 or k * 512) the
 * step gave it, FirPos() now, sound blocks emitted since it joined (the seq of its next wf_pkt_t, rx_waterfall.cpp:1635). */
int kg_rxbank_audio_map(kg_rxbank *bank, int32_t *nrec, int32_t *nfir, int32_t *fir_pos, uint32_t *snd_seq);
/* wf_pkt_t header fields of receiver rx (x_bin_server, zoom, compression); seq is the bank's sound sequence number. */
int kg_rxbank_set_wf_pkt(kg_rxbank *bank, int rx, uint32_t x_bin_server, uint32_t zoom, int use_compression);
/* snd_service() unpack parameters (default: rescale of rx/data_pump.cpp:73-74, no DC offset, no inversion) */
/* "SET little-endian" of a connection (rx/rx_sound.cpp:1076-1096): the byte order of receiver rx's IQ-mode payload (default:
 * network order).  A receiver whose kg_post mode is stereo (IS_STEREO: KG_POST_IQ, KG_POST_SAS, KG_POST_QAM) gets its sound blocks
 * as IQ payload rows (bufs.iq_pay; SAS / QAM: their (L, R) pair, rx_sound.cpp:1047-1049), the others as ADPCM rows (bufs.adpcm);
 * the mode is read at every step. */
int kg_rxbank_set_little_endian(kg_rxbank *bank, int rx, int little_endian);
int kg_rxbank_set_unpack(kg_rxbank *bank, float rescale, float dc_i, float dc_q, int spectral_inversion);

typedef struct {
    uint64_t step;         /* steps taken before this one */
    int32_t nframes;       /* waterfall frames (= rows = packets) of this step: kg_rxbank_frame_map says whose */
    /* the next four: of the lowest-numbered ACTIVE receiver (all receivers of a bank that was never joined into agree);
     * per receiver: kg_rxbank_audio_map */
    int32_t nrec;          /* rx_iq_t records */
    int32_t nfir;          /* CFastFIR outputs: 0 or k * 512 (k sound blocks: s16 / adpcm rows hold k * 512 / k * 256) */
    int32_t fir_pos;       /* FirPos() after the step */
    uint32_t snd_seq;      /* sound blocks emitted before this step = the seq of this step's wf_pkt_t (rx_waterfall.cpp:1635) */
    int32_t table_bytes;   /* what the step's one upload carried */
    int32_t nmoves;        /* overlapped rings wrapped this step */
} kg_rxbank_step_info;
/* One step: n = adc_samples_per_step samples at d_adc (device) through every receiver.  Enqueue only (the host returns
 * after some thirty launches; kg_rxbank_poll / _sync say when the work is done).  adc_ready_event: a hipEvent_t recorded
 * behind the writer of d_adc, or NULL.  info may be NULL.  A negative return from the PLAN half of the call (bad state, a
 * receiver without a waterfall setting) leaves the bank as it was; an error of the HIP runtime while the step is being
 * enqueued leaves it half-advanced: destroy the bank.  One host thread per bank. */
int kg_rxbank_step(kg_rxbank *bank, const void *d_adc, void *adc_ready_event, kg_rxbank_step_info *info);
/* The host runs at most KG_RXBANK_SLOTS steps ahead of the GPU: kg_rxbank_step(k) returns only when step k - 8 has
 * completed on the device.  An ADC ring of KG_RXBANK_SLOTS + 1 buffers therefore needs NO device-side ordering of its writer:
 * when step k has been enqueued, the buffer step k + 1 will use was last read by step k - 8, which is done (measured: the
 * resident step time with every block copied from pinned host memory, 1.25 ms).  A shorter ring orders its writer with
 * kg_rxbank_adc_done: `stream` (hipStream_t) waits until the readers of the ADC block of the step `steps_back` steps ago are
 * done (1: the last step; 2: the one before it = the buffer a double-buffered ring refills next; at most 8) -- correct, but a
 * wait enqueued on a stream that shares a hardware queue with one of the bank's holds that queue until the old step has
 * completed (measured with two buffers: 1.47 ms per step instead of 1.25). */
#define KG_RXBANK_SLOTS 8
int kg_rxbank_adc_done(kg_rxbank *bank, void *stream, int steps_back);
int kg_rxbank_poll(kg_rxbank *bank);          /* 1 = all streams idle, 0 = busy, <0 error */
/* 1: the next kg_rxbank_step will not wait for its table slot; 0: it would sleep until the step KG_RXBANK_SLOTS back has run --
 * a cooperative host (the reference's coroutine server, NextTask) yields and asks again. */
int kg_rxbank_ready(kg_rxbank *bank);
int kg_rxbank_sync(kg_rxbank *bank);
/* Frame f of the last step belongs to receiver rx_of_frame[f], was read at wf_iq + frame_off[f] pairs, and its packet has
 * pkt_bytes[f] bytes on the wire (arrays of nrx entries, any may be NULL).  Returns nframes. */
int kg_rxbank_frame_map(kg_rxbank *bank, int32_t *rx_of_frame, uint64_t *frame_off, int32_t *pkt_bytes);
/* The bank's device buffers (valid until kg_rxbank_destroy; read them after kg_rxbank_sync or behind the bank's streams).  A step
 * writes, of receiver rx's rows, rx_raw / rx_in up to its nrec records, fir_out up to its nfir samples, then s16 and adpcm (the real
 * modes) or iq_pay (the stereo modes) and agc (every mode but SSB) up to nfir; of frame f < nframes its 1024-byte row and pkt_bytes[f]
 * bytes of its packet.  Nothing beyond those counts, no row of a receiver that left, no slot beyond nframes, and a step reads none of
 * these buffers' earlier contents (wf_iq excepted: the samplers' rings). */
typedef struct {
    void *wf_iq;   size_t wf_iq_stride;   /* [nrx][wf_iq_stride] iq_t: the samplers' rows (one-shot: pairs 0..8191) */
    void *wf_rows;                        /* [frame][1024] u8 */
    void *wf_pkts; size_t wf_pkt_stride;  /* [frame][wf_pkt_stride] wf_pkt_t bytes */
    void *rx_raw;  size_t rx_stride;      /* [nrx][rx_stride] rx_iq_t (6 bytes each) */
    void *rx_in;                          /* [nrx][rx_stride] TYPECPX: what CFastFIR was fed */
    void *fir_out; size_t fir_stride;     /* [nrx][fir_stride] TYPECPX */
    void *s16;                            /* [nrx][fir_stride] int16: CAgc / detector output */
    void *adpcm;                          /* [nrx][fir_stride / 2] bytes: the real modes' ADPCM payload */
    void *agc;                            /* [nrx][fir_stride] TYPECPX: the AGC's output (rx->agc_samples_c; every mode but SSB) */
    void *iq_pay;                         /* [nrx][4 fir_stride] bytes: the IQ mode's payload, (s2_t) re, (s2_t) im per sample */
} kg_rxbank_bufs;
int kg_rxbank_buffers(kg_rxbank *bank, kg_rxbank_bufs *out);
/* Where the host's share of the steps since the last call went, by phase (microseconds per step, text). */
int kg_rxbank_host_profile(kg_rxbank *bank, char *buf, size_t len);

#ifdef __cplusplus
}
#endif
#endif /* KIWIGPU_H */
