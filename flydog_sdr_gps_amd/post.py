"""Host-side mirror of what consumes the CFastFIR output in c2s_sound(), over the C ABI.

Reference                                                              here
  sMeterAlpha / sMeterAvg_dB loop   rx/rx_sound.cpp:248-250, 676-696 -> Post.set_smeter, Post.smeter
  m_Agc[ch].SetParameters(...)      rx/CuteSDR/agc.cpp:98-163        -> Post.set_agc
  m_Agc[ch].GetDelaySamples()       rx/CuteSDR/agc.h:27              -> Post.agc_delay
  m_Agc[ch].ProcessData(n, in, out) rx/CuteSDR/agc.cpp:259-292       -> Post.process (modes IQ / SSB)
  AM detector + DC removal          rx/rx_sound.cpp:766-783          -> Post.process (mode AM)
  m_AM_FIR.InitLPFilter(...)        rx/rx_sound_cmd.cpp:268-282      -> Post.set_am_passband (Post.cfir_init_lp)
  m_AM_FIR.ProcessFilter            rx/rx_sound.cpp:787              -> Post.process (mode AM, s16)
  NBFM fmdemod_quadri + clipper     rx/rx_sound.cpp:845-875          -> Post.process (mode NBFM)
  m_Squelch.SetupParameters / SetSquelch / Reset
                                    rx/rx_sound.cpp:261-262, rx/rx_sound_cmd.cpp:238,430
                                                                     -> Post.squelch_setup / squelch_set / squelch_reset
  m_Squelch.PerformFMSquelch        rx/rx_sound.cpp:876-877          -> Post.process (mode NBFM, s16), Post.squelch_state
  "SET de_emp=%d nfm=%d"            rx/rx_sound_cmd.cpp:543-585      -> Post.set_de_emp (tables: deemp.py)
  m_*_deemp_FIR.ProcessFilter       rx/rx_sound.cpp:898-907          -> Post.process (s16, in place)
  wdsp_SAM_demod (SAM/SAU/SAL/SAS/QAM) rx/rx_sound.cpp:791-806      -> Post.process (modes SAM .. QAM)
  wdsp_SAM_demod_init()             rx/wdsp/SAM_demod.cpp:154-163    -> Post.sam_setup
  wdsp_SAM_PLL(type), SET sam_pll=  SAM_demod.cpp:113-152            -> Post.sam_pll
  s->SAM_mparam                     rx/rx_sound_cmd.cpp:216          -> Post.set_sam_mparam
  wdsp_SAM_carrier(), s->isChanNull SAM_demod.cpp:165-170            -> Post.sam_state
  "SET nr algo=" / "SET nr type= en=" / "SET nr type= param= pval="
                                    rx/rx_sound_cmd.cpp:464-523      -> Post.set_nr_algo / set_nr_enable / set_nr_param
  the noise-reduction switch (NR_WDSP: wdsp_ANR_filter, NR_ORIG: CLMS::ProcessFilter)
                                    rx/rx_sound.cpp:933-949          -> Post.process (s16, in place), Post.nr_process, Post.nr_state
  "SET nr algo=3", nr_spectral_init, s->norm_locut / norm_hicut
                                    rx/rx_sound_cmd.cpp:464-471, :520, :252-266
                                                                     -> Post.nrs_select / set_nr_param / nrs_passband / nrs_setup
  NR_SPECTRAL: nr_spectral_process  rx/rx_sound.cpp:945-947, rx/Teensy/NR_spectral.cpp
                                                                     -> Post.process (s16, in place), Post.nrs_process, Post.nrs_state
  nb_Wild_init (`SET nb type=0 param= pval=` under NB_WILD)
                                    rx/rx_sound_cmd.cpp:498, rx/Teensy/NB_Wild.cpp:38-46
                                                                     -> Post.nbw_init
  s->nb_enable[NB_BLANKER] && s->nb_algo == NB_WILD
                                    rx/rx_sound.cpp:924-929          -> Post.set_nbw
  NB_WILD: nb_Wild_process          rx/rx_sound.cpp:929, rx/Teensy/NB_Wild.cpp:60-261
                                                                     -> Post.process (s16, in place), Post.nbw_process, Post.nbw_state
"""
import ctypes as C

import numpy as np

from ._lib import Context, check, ptr, own_rows

MODE_IQ, MODE_SSB, MODE_AM, MODE_NBFM = range(4)      # KG_POST_* of include/kiwigpu.h
MODE_SAM, MODE_SAU, MODE_SAL, MODE_SAS, MODE_QAM = range(4, 9)
SAM_MODES = (MODE_SAM, MODE_SAU, MODE_SAL, MODE_SAS, MODE_QAM)
STEREO_MODES = (MODE_IQ, MODE_SAS, MODE_QAM)          # IS_STEREO (rx/mode.h:45-55): the packet carries IQ payload
PLL_RESET, PLL_DX, PLL_MED, PLL_FAST = -1, 0, 1, 2    # rx/wdsp/wdsp.h:14
CHAN_NULL_LSB, CHAN_NULL_USB, FADE_LEVELER, DC_BLOCK = 1, 2, 4, 8    # SAM_mparam bits, wdsp.h:5-10
MAX_SAMPLES = 1024                                    # KG_POST_MAX_SAMPLES
CFIR_AM, CFIR_DEEMP_NFM, CFIR_DEEMP_AM_SSB, CFIR_SQUELCH_HP = range(4)  # KG_CFIR_*
CFIR_REAL_REAL, CFIR_REAL_MONO16, CFIR_MONO16_MONO16 = range(3)        # the ProcessFilter overloads
NR_OFF, NR_WDSP, NR_ORIG, NR_SPECTRAL = range(4)      # KG_NR_* (nr_algo_e, rx/rx_noise.h:9); NR_SPECTRAL: Post.nrs_select
NR_DENOISE, NR_AUTONOTCH = 0, 1                       # nr_type_e
NR_DELAY, NR_BETA, NR_DECAY = 0, 1, 2                 # NR_ORIG's parameters (extensions/noise_filter/noise_filter.h)
NR_TAPS, NR_DLY, NR_GAIN, NR_LEAKAGE = 0, 1, 2, 3     # NR_WDSP's
NR_PARAMS = 8
NR_S_GAIN, NR_ALPHA, NR_ASNR = 0, 1, 2                # NR_SPECTRAL's (either type index reaches the one state)
NRS_BLOCK = 512                                       # nr_spectral_process runs on blocks of FFT_FULL samples
NRS_ARRAYS = ("last_sample_buffer", "last_iFFT_result", "NR_Nest", "xt", "pslp", "NR_SNR_post", "NR_SNR_prio", "NR_Hk_old", "NR_G")
NRS_VAD_HIGH_MIN, NRS_VAD_LOW_MAX = 17, 244           # the passbands NR_spectral.cpp's smoothing loops stay inside their arrays on
NB_THRESH, NB_TAPS, NB_SAMPLES = 0, 1, 2              # NB_WILD's parameters (extensions/noise_blank/noise_blank.h)
NBW_BLOCK = 512                                       # nb_Wild_process runs on the call site's ns_out
NBW_MAX_ORDER, NBW_MAX_IMPULSE_LEN, NBW_HIST = 40, 41, 120    # NB_Wild.cpp:23-24; the most a call carries to the next


def nbw_delay(taps, impulse_samples):
    """order + PL: by how many samples the Wild blanker's output lags its input (NB_Wild.cpp:66-68, :239)"""
    return int(taps) + ((int(impulse_samples) | 1) - 1) // 2


def nrs_norm_passband(locut, hicut):
    """rx_sound_cmd.cpp:252-266 from the clamped cuts -> (norm_locut, norm_hicut) as float32"""
    locut, hicut = float(locut), float(hicut)
    if locut <= 0 and hicut >= 0:
        return np.float32(0.0), np.float32(max(-locut, hicut))
    if locut > 0:
        return np.float32(locut), np.float32(hicut)
    return np.float32(-hicut), np.float32(-locut)


def nrs_vad_bins(norm_locut, norm_hicut, snd_rate):
    """NR_spectral.cpp:214-238 -> (VAD_low, VAD_high); float32 arithmetic as there"""
    binw = np.float32(snd_rate) / np.float32(512)
    lo = int(np.floor(np.float32(norm_locut) / binw))
    hi = int(np.ceil(np.float32(norm_hicut) / binw))
    if lo == hi:
        hi += 1
    lo = 1 if lo < 1 else min(lo, 254)
    hi = 2 if hi < 2 else min(hi, 256)
    return lo, hi


def nrs_passband_ok(locut, hicut, snd_rate):
    lo, hi = nrs_vad_bins(*nrs_norm_passband(locut, hicut), snd_rate)
    return hi >= NRS_VAD_HIGH_MIN and lo <= NRS_VAD_LOW_MAX


class Post:
    """S-meter + CAgc + detector state of nchan receiver channels on the GPU (kg_post)."""

    def __init__(self, ctx=None, nchan=4, device=0):
        self.ctx = ctx if ctx is not None else Context(device)
        self.lib = self.ctx.lib
        self.nchan = nchan
        h = C.c_void_p()
        check(self.lib.kg_post_create(self.ctx.h, int(nchan), C.byref(h)), "kg_post_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None) and not getattr(self, "_borrowed", False):          # an object must not outlive its context
                self.lib.kg_post_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_agc(self, ch, agc_on, use_hang, threshold, manual_gain, slope, decay, sample_rate):
        check(self.lib.kg_post_set_agc(self.h, int(ch), int(bool(agc_on)), int(bool(use_hang)), int(threshold),
                                       int(manual_gain), int(slope), int(decay), float(sample_rate)),
              "kg_post_set_agc")

    def agc_delay(self, ch):
        return check(self.lib.kg_post_agc_delay(self.h, int(ch)), "kg_post_agc_delay")

    def set_smeter(self, ch, frate):
        check(self.lib.kg_post_set_smeter(self.h, int(ch), float(frate)), "kg_post_set_smeter")

    def set_mode(self, ch, mode):
        check(self.lib.kg_post_set_mode(self.h, int(ch), int(mode)), "kg_post_set_mode")

    def reset(self, ch):
        check(self.lib.kg_post_reset(self.h, int(ch)), "kg_post_reset")

    # ---- the synchronous-AM demodulator (rx/wdsp/SAM_demod.cpp) ----
    def sam_setup(self, ch, snd_rate):
        check(self.lib.kg_post_sam_setup(self.h, int(ch), int(snd_rate)), "kg_post_sam_setup")

    def sam_pll(self, ch, pll_type):
        check(self.lib.kg_post_sam_pll(self.h, int(ch), int(pll_type)), "kg_post_sam_pll")

    def set_sam_mparam(self, ch, mparam):
        check(self.lib.kg_post_set_sam_mparam(self.h, int(ch), int(mparam)), "kg_post_set_sam_mparam")

    def sam_state(self, chans):
        """-> (SAM_carrier float32[n] (NaN -> 0), isChanNull int32[n], phzerror float32[n]) after the last pass"""
        chans = np.ascontiguousarray(chans, np.int32)
        car = np.zeros(chans.size, np.float32)
        null = np.zeros(chans.size, np.int32)
        phz = np.zeros(chans.size, np.float32)
        check(self.lib.kg_post_sam_state(self.h, ptr(chans), chans.size, ptr(car), ptr(null), ptr(phz)), "kg_post_sam_state")
        return car, null, phz

    # ---- CFir objects (rx/CuteSDR/fir.cpp) ----
    # ---- the noise-reduction switch (rx/rx_sound.cpp:933-949) ----
    def set_nr_algo(self, ch, algo):
        """`SET nr algo=`: the algo, both enables cleared, no filter state touched"""
        check(self.lib.kg_post_set_nr_algo(self.h, int(ch), int(algo)), "kg_post_set_nr_algo")

    def set_nr_enable(self, ch, nr_type, en):
        check(self.lib.kg_post_set_nr_enable(self.h, int(ch), int(nr_type), int(en)), "kg_post_set_nr_enable")

    def set_nr_param(self, ch, nr_type, param, pval):
        """`SET nr type= param= pval=`: stores the float and re-initialises that type of the current algo from its whole vector"""
        check(self.lib.kg_post_set_nr_param(self.h, int(ch), int(nr_type), int(param), float(np.float32(pval))), "kg_post_set_nr_param")

    def nr_process_dev(self, chans, nr_type, d_in, in_stride, nsamps, d_out, out_stride=None):
        chans = np.ascontiguousarray(chans, np.int32)
        check(self.lib.kg_post_nr_process_dev(self.h, ptr(chans), chans.size, int(nr_type), ptr(int(d_in)), int(in_stride), int(nsamps),
                                              ptr(int(d_out)), int(out_stride if out_stride is not None else nsamps)),
              "kg_post_nr_process_dev")

    def nr_process(self, chans, nr_type, x):
        """x: int16 [len(chans), n] (host).  -> int16 [len(chans), n]: the filter of nr_type under each channel's algo"""
        own_rows(self, "nr_process()")
        chans = np.ascontiguousarray(chans, np.int32)
        x = np.ascontiguousarray(x, np.int16).reshape(chans.size, -1)
        n = x.shape[1]
        y = np.empty_like(x)
        ctx = self.ctx
        b = ctx.alloc(x.nbytes)
        try:
            ctx.upload(b, x)
            self.nr_process_dev(chans, nr_type, b, n, n, b, n)
            ctx.sync()
            ctx.download(b, y)
        finally:
            ctx.free(b)
        return y

    def nr_state(self, chans, nr_type, weights=False):
        """-> dict: anr_i int32[n, 3] (in_idx, taps, delay), anr_f float32[n, 2] (lidx, ngamma), lms_i int32[n, 3] (dlp, dlen, nr_type)
        and with weights=True anr_w float32[n, 512], lms_coef float32[n, 121]"""
        chans = np.ascontiguousarray(chans, np.int32)
        n = chans.size
        r = dict(anr_i=np.zeros((n, 3), np.int32), anr_f=np.zeros((n, 2), np.float32), lms_i=np.zeros((n, 3), np.int32))
        if weights:
            r.update(anr_w=np.zeros((n, 512), np.float32), lms_coef=np.zeros((n, 121), np.float32))
        check(self.lib.kg_post_nr_state(self.h, ptr(chans), n, int(nr_type), ptr(r["anr_i"]), ptr(r["anr_f"]), ptr(r["lms_i"]),
                                        ptr(r.get("anr_w")), ptr(r.get("lms_coef"))), "kg_post_nr_state")
        return r

    # ---- NR_SPECTRAL (rx/Teensy/NR_spectral.cpp) ----
    def nrs_select(self, ch):
        """`SET nr algo=3`: NR_SPECTRAL, both enables cleared.  Refused while the channel's passband (nrs_passband) is one on which
        the reference indexes outside its arrays.  Any set_nr_algo afterwards leaves it."""
        check(self.lib.kg_post_nrs_select(self.h, int(ch)), "kg_post_nrs_select")

    def nrs_setup(self, snd_rate):
        """the reference's snd_rate for NR_SPECTRAL (tinc .. ap, the bin width): 12000 until called"""
        check(self.lib.kg_post_nrs_setup(self.h, int(snd_rate)), "kg_post_nrs_setup")

    def nrs_passband(self, ch, locut, hicut):
        """s->norm_locut / norm_hicut from the clamped cuts of `SET mod= low_cut= high_cut=`"""
        check(self.lib.kg_post_nrs_passband(self.h, int(ch), float(locut), float(hicut)), "kg_post_nrs_passband")

    def nrs_process_dev(self, chans, d_in, in_stride, nsamps, d_out, out_stride=None):
        chans = np.ascontiguousarray(chans, np.int32)
        check(self.lib.kg_post_nrs_process_dev(self.h, ptr(chans), chans.size, ptr(int(d_in)), int(in_stride), int(nsamps),
                                               ptr(int(d_out)), int(out_stride if out_stride is not None else nsamps)),
              "kg_post_nrs_process_dev")

    def nrs_process(self, chans, x, in_place=True):
        """x: int16 [len(chans), n] (host), n a multiple of 512.  -> int16 [len(chans), n]: nr_spectral_process per 512 samples"""
        own_rows(self, "nrs_process()")
        chans = np.ascontiguousarray(chans, np.int32)
        x = np.ascontiguousarray(x, np.int16).reshape(chans.size, -1)
        n = x.shape[1]
        y = np.empty_like(x)
        ctx = self.ctx
        b = ctx.alloc(x.nbytes)
        o = b if in_place else ctx.alloc(x.nbytes)
        try:
            ctx.upload(b, x)
            self.nrs_process_dev(chans, b, n, n, o, n)
            ctx.sync()
            ctx.download(o, y)
        finally:
            ctx.free(b)
            if not in_place:
                ctx.free(o)
        return y

    def nrs_state(self, chans):
        """-> dict: ints int32[n, 4] (first_time, init_counter, VAD_low, VAD_high), scalars float32[n, 8] (final_gain, alpha, asnr,
        xih1, xih1r, pfac, norm_locut, norm_hicut), rate float32[6] (tinc, tax, tap, ax, ap, snr_prio_min), arrays float32[n, 9, 256]
        in NRS_ARRAYS' order"""
        chans = np.ascontiguousarray(chans, np.int32)
        n = chans.size
        r = dict(ints=np.zeros((n, 4), np.int32), scalars=np.zeros((n, 8), np.float32), rate=np.zeros(6, np.float32),
                 arrays=np.zeros((n, 9, 256), np.float32))
        check(self.lib.kg_post_nrs_state(self.h, ptr(chans), n, ptr(r["ints"]), ptr(r["scalars"]), ptr(r["rate"]), ptr(r["arrays"])),
              "kg_post_nrs_state")
        return r

    # ---- NB_WILD (rx/Teensy/NB_Wild.cpp) ----
    def nbw_init(self, ch, nb_param):
        """nb_Wild_init: the state and its history zeroed, then thresh, taps, impulse_samples from nb_param (NB_THRESH, NB_TAPS,
        NB_SAMPLES; up to NR_PARAMS values, the rest 0).  Never refused while the stage is off."""
        v = np.zeros(NR_PARAMS, np.float32)
        p = np.asarray(nb_param, np.float32).ravel()
        v[:p.size] = p
        check(self.lib.kg_post_nbw_init(self.h, int(ch), ptr(v)), "kg_post_nbw_init")

    def set_nbw(self, ch, on):
        """the stage's switch (nb_enable[NB_BLANKER] && nb_algo == NB_WILD); reset() clears it"""
        check(self.lib.kg_post_set_nbw(self.h, int(ch), int(bool(on))), "kg_post_set_nbw")

    def nbw_process_dev(self, chans, d_in, in_stride, nsamps, d_out, out_stride=None):
        chans = np.ascontiguousarray(chans, np.int32)
        check(self.lib.kg_post_nbw_process_dev(self.h, ptr(chans), chans.size, ptr(int(d_in)), int(in_stride), int(nsamps),
                                               ptr(int(d_out)), int(out_stride if out_stride is not None else nsamps)),
              "kg_post_nbw_process_dev")

    def nbw_process(self, chans, x, in_place=True):
        """x: int16 [len(chans), n] (host), n a multiple of 512.  -> int16 [len(chans), n]: nb_Wild_process per 512 samples"""
        own_rows(self, "nbw_process()")
        chans = np.ascontiguousarray(chans, np.int32)
        x = np.ascontiguousarray(x, np.int16).reshape(chans.size, -1)
        n = x.shape[1]
        y = np.empty_like(x)
        ctx = self.ctx
        b = ctx.alloc(x.nbytes)
        o = b if in_place else ctx.alloc(x.nbytes)
        try:
            ctx.upload(b, x)
            self.nbw_process_dev(chans, b, n, n, o, n)
            ctx.sync()
            ctx.download(o, y)
        finally:
            ctx.free(b)
            if not in_place:
                ctx.free(o)
        return y

    def nbw_state(self, chans):
        """-> dict: ints int32[n, 3] (taps, impulse_samples, the switch), thresh float32[n], hist float32[n, 120] (working_buffer's
        head: a call writes its first 2 * order + 2 * PL, the rest is 0)"""
        chans = np.ascontiguousarray(chans, np.int32)
        n = chans.size
        ints = np.zeros((n, 3), np.int32)
        flts = np.zeros((n, 1 + NBW_HIST), np.float32)
        check(self.lib.kg_post_nbw_state(self.h, ptr(chans), n, ptr(ints), ptr(flts)), "kg_post_nbw_state")
        return dict(ints=ints, thresh=flts[:, 0].copy(), hist=flts[:, 1:].copy())

    def cfir_init_lp(self, ch, which, numtaps, scale, astop, fpass, fstop, fs):
        """CFir::InitLPFilter -> tap count"""
        return check(self.lib.kg_post_cfir_init_lp(self.h, int(ch), int(which), int(numtaps), float(scale), float(astop), float(fpass),
                                                   float(fstop), float(fs)), "kg_post_cfir_init_lp")

    def cfir_init_const(self, ch, which, coef, fs=12000.0):
        """CFir::InitConstFir -> tap count"""
        coef = np.ascontiguousarray(coef, np.float32)
        return check(self.lib.kg_post_cfir_init_const(self.h, int(ch), int(which), coef.size, ptr(coef), float(fs)),
                     "kg_post_cfir_init_const")

    def cfir_taps(self, ch, which):
        taps = np.zeros(97, np.float32)
        n = check(self.lib.kg_post_cfir_get_taps(self.h, int(ch), int(which), ptr(taps)), "kg_post_cfir_get_taps")
        return taps[:n].copy()

    def cfir_process(self, chans, which, kind, x):
        """m_*_FIR[ch].ProcessFilter on host rows x [len(chans), n] (float32, or int16 for CFIR_MONO16_MONO16)."""
        own_rows(self, "cfir_process()")
        chans = np.ascontiguousarray(chans, np.int32)
        x = np.ascontiguousarray(x, np.int16 if kind == CFIR_MONO16_MONO16 else np.float32).reshape(chans.size, -1)
        n = x.shape[1]
        out = np.zeros((chans.size, n), np.float32 if kind == CFIR_REAL_REAL else np.int16)
        ctx = self.ctx
        bi, bo = ctx.alloc(x.nbytes), ctx.alloc(out.nbytes)
        try:
            ctx.upload(bi, x)
            check(self.lib.kg_post_cfir_process_dev(self.h, ptr(chans), chans.size, int(which), int(kind), ptr(int(bi)), n, n, ptr(int(bo)), n),
                  "kg_post_cfir_process_dev")
            ctx.sync()
            ctx.download(bo, out)
        finally:
            ctx.free(bi)
            ctx.free(bo)
        return out

    def squelch_perform(self, chans, x):
        """m_Squelch[ch].PerformFMSquelch on host rows x float32 [len(chans), n] -> (mono16 [len(chans), n], nsq_nc_sq int32[len(chans)])"""
        own_rows(self, "squelch_perform()")
        chans = np.ascontiguousarray(chans, np.int32)
        x = np.ascontiguousarray(x, np.float32).reshape(chans.size, -1)
        n = x.shape[1]
        out = np.zeros((chans.size, n), np.int16)
        ctx = self.ctx
        bi, bo = ctx.alloc(x.nbytes), ctx.alloc(out.nbytes)
        try:
            ctx.upload(bi, x)
            check(self.lib.kg_post_squelch_perform_dev(self.h, ptr(chans), chans.size, ptr(int(bi)), n, n, ptr(int(bo)), n),
                  "kg_post_squelch_perform_dev")
            ctx.sync()
            ctx.download(bo, out)
        finally:
            ctx.free(bi)
            ctx.free(bo)
        return out, self.squelch_state(chans)[0]

    def set_am_passband(self, ch, locut, hicut, frate):
        """The m_AM_FIR design of a passband change (rx/rx_sound_cmd.cpp:268-282) -> tap count"""
        return check(self.lib.kg_post_set_am_passband(self.h, int(ch), float(locut), float(hicut), float(frate)), "kg_post_set_am_passband")

    def set_deemp(self, ch, nfm, de_emp):
        check(self.lib.kg_post_set_deemp(self.h, int(ch), int(bool(nfm)), int(de_emp)), "kg_post_set_deemp")

    def set_de_emp(self, ch, de_emp, nfm, snd_rate_12k=True, frate=None):
        """`SET de_emp=<de_emp> nfm=<nfm>` as rx/rx_sound_cmd.cpp:543-585 handles it: the flag, and for de_emp 1 / 2 the
        coefficients of rx/rx_filter.h's table into the mode's filter (InitConstFir clears its samples)."""
        from . import deemp
        self.set_deemp(ch, nfm, de_emp)
        if de_emp:
            rate = frate if frate is not None else (12000.0 if snd_rate_12k else 20250.0)
            self.cfir_init_const(ch, CFIR_DEEMP_NFM if nfm else CFIR_DEEMP_AM_SSB, deemp.table(nfm, snd_rate_12k)[de_emp - 1], rate)

    # ---- CSquelch (rx/CuteSDR/squelch.cpp) ----
    def squelch_setup(self, ch, samplerate):
        check(self.lib.kg_post_squelch_setup(self.h, int(ch), float(samplerate)), "kg_post_squelch_setup")

    def squelch_set(self, ch, value, squelch_max=0):
        check(self.lib.kg_post_squelch_set(self.h, int(ch), int(value), int(squelch_max)), "kg_post_squelch_set")

    def squelch_reset(self, ch):
        check(self.lib.kg_post_squelch_reset(self.h, int(ch)), "kg_post_squelch_reset")

    def squelch_state(self, chans):
        """-> (nsq_nc_sq int32[n], squelched int32[n], m_SquelchAve float32[n]) after the last pass"""
        chans = np.ascontiguousarray(chans, np.int32)
        rc = np.zeros(chans.size, np.int32)
        sq = np.zeros(chans.size, np.int32)
        ave = np.zeros(chans.size, np.float32)
        check(self.lib.kg_post_squelch_state(self.h, ptr(chans), chans.size, ptr(rc), ptr(sq), ptr(ave)), "kg_post_squelch_state")
        return rc, sq, ave

    def process_dev(self, chans, d_fir, in_stride, nsamps, d_s16=0, d_demod=0, d_agc=0, out_stride=None):
        chans = np.ascontiguousarray(chans, np.int32)
        check(self.lib.kg_post_process_dev(self.h, ptr(chans), chans.size, ptr(int(d_fir)), int(in_stride),
                                           int(nsamps), ptr(int(d_s16)) if d_s16 else None,
                                           ptr(int(d_demod)) if d_demod else None,
                                           ptr(int(d_agc)) if d_agc else None,
                                           int(out_stride if out_stride is not None else nsamps)),
              "kg_post_process_dev")

    def process(self, chans, x):
        """x: complex64 [len(chans), n] FIR output (host).  -> (s16 int16, demod float32, agc complex64),
        each [len(chans), n]; a row is meaningful where the channel's mode produces it."""
        own_rows(self, "process()")
        chans = np.ascontiguousarray(chans, np.int32)
        x = np.ascontiguousarray(x, np.complex64).reshape(chans.size, -1)
        n = x.shape[1]
        s16 = np.zeros((chans.size, n), np.int16)
        demod = np.zeros((chans.size, n), np.float32)
        agc = np.zeros((chans.size, n), np.complex64)
        ctx = self.ctx
        bufs = [ctx.alloc(a.nbytes) for a in (x, s16, demod, agc)]
        try:
            ctx.upload(bufs[0], x)
            for b, a in zip(bufs[1:], (s16, demod, agc)):
                ctx.upload(b, a)
            self.process_dev(chans, bufs[0], n, n, bufs[1], bufs[2], bufs[3], n)
            ctx.sync()
            for b, a in zip(bufs[1:], (s16, demod, agc)):
                ctx.download(b, a)
        finally:
            for b in bufs:
                ctx.free(b)
        return s16, demod, agc

    def smeter(self, chans):
        """-> (sMeterAvg_dB float32[len(chans)], taps float32[len(chans), 2])"""
        chans = np.ascontiguousarray(chans, np.int32)
        avg = np.zeros(chans.size, np.float32)
        taps = np.zeros((chans.size, 2), np.float32)
        check(self.lib.kg_post_smeter(self.h, ptr(chans), chans.size, ptr(avg), ptr(taps)), "kg_post_smeter")
        return avg, taps


MATH_LOG10F, MATH_POWF, MATH_EXPF, MATH_SINF, MATH_COSF = 0, 1, 2, 3, 4          # KG_MATH_*


def math_dev(ctx, fn, x=None, first_bits=0, n=None, base=10.0):
    """kg_math_dev: the device's log10f / powf(base, .) / expf -- the host libm's algorithms, csrc/kg_libm.h -- over an array (x), or
    over the n floats whose bit patterns start at first_bits.  -> float32[n]"""
    if x is not None:
        x = np.ascontiguousarray(x, np.float32)
        n = x.size
    n = int(n)
    out = np.empty(n, np.float32)
    d_y = ctx.alloc(4 * n)
    d_x = ctx.alloc(4 * n) if x is not None else 0
    try:
        if x is not None:
            ctx.upload(d_x, x)
        check(ctx.lib.kg_math_dev(ctx.h, int(fn), float(base), C.c_void_p(d_x) if d_x else None, int(first_bits) & 0xFFFFFFFF, n,
                                  C.c_void_p(d_y)), "kg_math_dev")
        ctx.sync()
        ctx.download(d_y, out)
    finally:
        ctx.free(d_y)
        if d_x:
            ctx.free(d_x)
    return out


def log10f(ctx, x=None, first_bits=0, n=None):
    return math_dev(ctx, MATH_LOG10F, x, first_bits, n)


def math_atan2f_dev(ctx, y, x):
    """kg_math_atan2f_dev: the device's atan2f (glibc 2.35's e_atan2f.c restated, csrc/kg_libm_trig.h) over float32 arrays -> float32"""
    y = np.ascontiguousarray(y, np.float32).reshape(-1)
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    assert y.size == x.size and y.size >= 1
    n = y.size
    out = np.empty(n, np.float32)
    d_y, d_x, d_o = ctx.alloc(4 * n), ctx.alloc(4 * n), ctx.alloc(4 * n)
    try:
        ctx.upload(d_y, y)
        ctx.upload(d_x, x)
        check(ctx.lib.kg_math_atan2f_dev(ctx.h, C.c_void_p(d_y), C.c_void_p(d_x), n, C.c_void_p(d_o)), "kg_math_atan2f_dev")
        ctx.sync()
        ctx.download(d_o, out)
    finally:
        for d in (d_y, d_x, d_o):
            ctx.free(d)
    return out
