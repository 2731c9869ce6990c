"""Host-side mirror of a bank of receivers over the C ABI (kg_rxbank, include/kiwigpu.h).

In the reference every connection runs two coroutines over what the data pump hands them:
  c2s_sound()      rx/rx_sound.cpp:333-601      in_samps -> CFastFIR -> S-meter / AGC / demod -> compression
  c2s_waterfall()  rx/rx_waterfall.cpp:930-1170  sample_wf() -> compute_frame() -> wf_pkt_t
RxBank is nrx such connections on one GPU; step() is ONE C call that enqueues a whole step of all of them.  The
per-seam objects (ddc, wf, rxddc, fir, post, adpcm) are the bank's own and are configured through the same wrapper
classes the single-seam tests use.
"""
import ctypes as C

import numpy as np

from . import nb as nb_mod
from . import post as post_mod
from . import wf as wf_mod
from ._lib import Context, borrow, check, load_library, ptr
from .ddc import RX_DECIM, RX_STD, Ddc, RxDdc, rx_phase_inc
from .nb import NoiseBlanker
from .post import Post
from .snd import RESCALE, FastFir
from .wf import Waterfall, WfParams
from .wire import Adpcm

WF_NFFT = 8192


class StepInfoC(C.Structure):
    _fields_ = [("step", C.c_uint64), ("nframes", C.c_int32), ("nrec", C.c_int32), ("nfir", C.c_int32),
                ("fir_pos", C.c_int32), ("snd_seq", C.c_uint32), ("table_bytes", C.c_int32), ("nmoves", C.c_int32)]


class BufsC(C.Structure):
    _fields_ = [("wf_iq", C.c_void_p), ("wf_iq_stride", C.c_size_t), ("wf_rows", C.c_void_p),
                ("wf_pkts", C.c_void_p), ("wf_pkt_stride", C.c_size_t), ("rx_raw", C.c_void_p), ("rx_stride", C.c_size_t),
                ("rx_in", C.c_void_p), ("fir_out", C.c_void_p), ("fir_stride", C.c_size_t), ("s16", C.c_void_p),
                ("adpcm", C.c_void_p), ("agc", C.c_void_p), ("iq_pay", C.c_void_p)]


ADC_CLOCK, UI_SRATE = 66.6666e6, 30.0e6


def survey_mix(nrx, first_rx=0, n=1 << 22, adc_clock=ADC_CLOCK, ui_srate=UI_SRATE):
    """BASELINE configs[3] as SURVEY.md 8(d) defines it: receiver k of the 1024 listens at f_k = 100 kHz + k 29 kHz, its
    waterfall at zoom 8 + (k mod 4) centred on f_k, audio passband 300-2700 Hz.  With a step of n = 2^22 ADC samples zooms
    8..10 (R = 128..512) fill a frame inside the step -- the non-overlapped frame -- and zoom 11 (R = 1024, 2^23 samples
    per frame) is what sample_wf() switches to overlapped sampling for (rx_waterfall.cpp:962-983).
    -> [(WfParams, overlapped, audio phase increment)] for receivers first_rx .. first_rx + nrx - 1"""
    hz_per_start = ui_srate / (1024 << 14)
    out = []
    for i in range(nrx):
        k = first_rx + i
        f = 100.0e3 + 29.0e3 * k
        zoom = 8 + k % 4
        span = ui_srate / (1 << zoom)
        p = WfParams.for_zoom(zoom, max(f - span / 2, 0.0) / hz_per_start, adc_clock=adc_clock, ui_srate=ui_srate)
        out.append((p, WF_NFFT * p.decim > n, rx_phase_inc(f, adc_clock)))
    return out


def light_mix(nrx, first_rx=0, n=1 << 22, adc_clock=ADC_CLOCK, ui_srate=UI_SRATE):
    """Rounds 2-4's receiver set, kept as a second named workload: zoom 1 + (k mod 10) (R = 1 .. 512, every frame one-shot),
    starts spread over the band, audio NCOs 10 Hz apart near 0.0123 f_adc."""
    hz_per_start = ui_srate / (1024 << 14)
    out = []
    for i in range(nrx):
        k = first_rx + i
        p = WfParams.for_zoom(1 + k % 10, (1.0e6 + 0.2e6 * (k % 97)) / hz_per_start, adc_clock=adc_clock, ui_srate=ui_srate)
        out.append((p, WF_NFFT * p.decim > n, rx_phase_inc(0.0123 * adc_clock - 1000.0 - 10.0 * k, adc_clock)))
    return out


MIXES = {"survey": survey_mix, "light": light_mix}


class RxBank:
    """nrx virtual receivers on one GPU (kg_rxbank)."""

    def __init__(self, nrx, n=1 << 22, device=0, rx_mode=RX_STD):
        self.lib = load_library()
        h = C.c_void_p()
        check(self.lib.kg_rxbank_create(int(device), int(nrx), int(n), int(rx_mode), C.byref(h)), "kg_rxbank_create")
        self.h, self.nrx, self.n, self.device = h, nrx, n, device
        self.ctx = Context.borrow(self.lib.kg_rxbank_ctx(h), device)
        self.ddc = borrow(Ddc, self.ctx, self.lib.kg_rxbank_ddc(h), nchan=nrx, max_samples=n)
        self.wf = borrow(Waterfall, self.ctx, self.lib.kg_rxbank_wf(h), nchan=nrx)
        self.rxddc = borrow(RxDdc, self.ctx, self.lib.kg_rxbank_rxddc(h), nchan=nrx, max_samples=n, mode=rx_mode)
        self.rxddc.decim = check(self.lib.kg_rxddc_decim(self.rxddc.h), "kg_rxddc_decim")
        self.rx_mode = int(rx_mode)
        self.fir = borrow(FastFir, self.ctx, self.lib.kg_rxbank_fir(h), nchan=nrx)
        self.post = borrow(Post, self.ctx, self.lib.kg_rxbank_post(h), nchan=nrx)
        self.adpcm = borrow(Adpcm, self.ctx, self.lib.kg_rxbank_adpcm(h), nchan=nrx)
        self.nb = borrow(NoiseBlanker, self.ctx, self.lib.kg_rxbank_nb(h), nchan=nrx)
        self.null_fir = borrow(FastFir, self.ctx, self.lib.kg_rxbank_null_fir(h), nchan=nrx)     # m_chan_null_FIR[]
        b = BufsC()
        check(self.lib.kg_rxbank_buffers(h, C.byref(b)), "kg_rxbank_buffers")
        self.bufs = b
        check(self.lib.kg_rxbank_set_unpack(h, RESCALE, 0.0, 0.0, 0), "kg_rxbank_set_unpack")
        self.params = [None] * nrx
        self.overlapped = [False] * nrx
        self.rx_inc = [0] * nrx
        self.little_endian = [False] * nrx
        self.audio = [None] * nrx                       # (mode, lo, hi, fs, de_emp, squelch) as set_audio configured it
        self.fs = ADC_CLOCK / self.rxddc.decim          # RX_DECIM (rx4 / rx8, rx14) or RX_DECIM_WIDE (rx3)

    def close(self):
        if getattr(self, "h", None):
            self.lib.kg_rxbank_destroy(self.h)
            self.h = None
            for o in (self.ddc, self.wf, self.rxddc, self.fir, self.null_fir, self.post, self.adpcm, self.nb, self.ctx):
                o.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- configuration (the reference's per-connection command handlers)
    def set_wf(self, rx, params, overlapped=False, interp=wf_mod.WF_MAX, window_func=wf_mod.WINF_HANNING, cic_comp=True,
               use_compression=True):
        """`SET zoom= start=` of receiver rx: DDC frequency / decimation / sampler mode, compute_frame()'s per-channel
        state, the wf_pkt_t header fields."""
        check(self.lib.kg_rxbank_set_wf(self.h, int(rx), int(params.i_offset) & ((1 << 48) - 1), int(params.decim),
                                        int(bool(overlapped))), "kg_rxbank_set_wf")
        self.wf.set_channel(rx, params, interp=interp, window_func=window_func, cic_comp=cic_comp, overlapped=overlapped)
        check(self.lib.kg_rxbank_set_wf_pkt(self.h, int(rx), int(params.start), int(params.zoom), int(bool(use_compression))),
              "kg_rxbank_set_wf_pkt")
        self.params[rx], self.overlapped[rx] = params, bool(overlapped)

    def set_audio(self, rx, phase_inc, lo=300.0, hi=2700.0, fs=None, mode=post_mod.MODE_SSB, de_emp=0, squelch=0, sam_mparam=0):
        """A connection's `SET mod= low_cut= high_cut= freq=`, `SET de_emp=`, `SET squelch=` for receiver rx: NCO, passband
        filter and the post-AM-detector filter designed with it (rx/rx_sound_cmd.cpp:268-282), AGC / S-meter / detector, the
        squelch of a new connection (rx/rx_sound.cpp:261-262) then the command's value, the mode's de-emphasis filter.
        mode: any post.MODE_* (the SAM family included: its PLL at the nominal snd_rate nearest fs, SAM_mparam = sam_mparam)."""
        fs = self.fs if fs is None else fs
        fmax = int(fs / 2 - 1)                          # the handler clamps the client's cuts first (rx_sound_cmd.cpp:248-250)
        lo, hi = max(float(lo), float(-fmax)), min(float(hi), float(fmax))
        self.rxddc.set_freq(rx, phase_inc)
        if not self.fir.setup(rx, lo, hi, 0.0, fs):
            raise ValueError("set_audio: CFastFIR::SetupParameters rejects the passband %g .. %g Hz at %g Hz (fastfir.cpp:193-200)" % (lo, hi, fs))
        self.null_fir.setup(rx, lo, hi, 0.0, fs)         # m_chan_null_FIR is designed with it (rx_sound_cmd.cpp:274-275)
        self.post.set_am_passband(rx, lo, hi, fs)
        self.post.set_agc(rx, True, False, -100, 50, 6, 1000, fs)
        self.post.set_smeter(rx, fs)
        self.post.sam_setup(rx, 12000 if abs(fs - 12000.0) < abs(fs - 20250.0) else 20250)
        self.post.set_sam_mparam(rx, sam_mparam)
        self.post.set_mode(rx, mode)
        self.post.reset(rx)
        # s->norm_locut / norm_hicut of the same command (rx_sound_cmd.cpp:252-266), which NR_SPECTRAL's passband bins follow; the
        # stage's snd_rate is one per kg_post (the reference's is a global): the nominal rate nearest fs
        nominal = 12000 if abs(fs - 12000.0) < abs(fs - 20250.0) else 20250
        if getattr(self, "_nrs_rate", 12000) != nominal:
            self.post.nrs_setup(nominal)
            self._nrs_rate = nominal
        self.post.nrs_passband(rx, lo, hi)
        self.post.squelch_setup(rx, fs)
        self.post.squelch_set(rx, 0, 0)
        if squelch:
            self.post.squelch_set(rx, squelch, 0)
        nfm = mode == post_mod.MODE_NBFM
        self.post.set_deemp(rx, True, 0)
        self.post.set_deemp(rx, False, 0)
        if de_emp:
            self.post.set_de_emp(rx, de_emp, nfm, snd_rate_12k=abs(fs - 12000.0) < abs(fs - 20250.0), frate=fs)
        self.rx_inc[rx] = int(phase_inc)
        self.audio[rx] = (int(mode), float(lo), float(hi), float(fs), int(de_emp), int(squelch))

    def configure(self, mix):
        """mix: [(WfParams, overlapped, audio phase increment)] per receiver (survey_mix / light_mix)."""
        self.wf.set_tables()
        for rx, (p, ov, inc) in enumerate(mix):
            self.set_wf(rx, p, ov)
            self.set_audio(rx, inc)

    # ---- connections come and go (kg_rxbank_join / _leave)
    def join(self, rx, wf_setting=None, phase_inc=None, **audio):
        """A connection starts on receiver rx: its state starts from zero, nobody else's is touched.  wf_setting = (WfParams,
        overlapped) and phase_inc / **audio (set_audio's arguments) configure it as its first commands would."""
        check(self.lib.kg_rxbank_join(self.h, int(rx)), "kg_rxbank_join")
        if wf_setting is not None:
            self.set_wf(rx, wf_setting[0], wf_setting[1])
        if phase_inc is not None:
            self.set_audio(rx, phase_inc, **audio)

    def set_nr(self, rx, algo, params=None, enable=(0, 0)):
        """The noise-reduction commands for receiver rx as a client sends them (rx/rx_sound_cmd.cpp:464-523): `SET nr algo=`, then
        every parameter one at a time (params: {type: [value of param 0, 1, ...]}), then the enables (denoise, auto-notch).  Call it
        after set_audio, whose connection start clears them (post.NR_* constants).  post.NR_SPECTRAL (`SET nr algo=3`) is selected
        through Post.nrs_select: its parameters (gain, alpha, active SNR) go through either type, its enables are not consulted, and
        it is refused on a passband (set_audio's lo / hi) on which the reference indexes outside its arrays."""
        if algo == post_mod.NR_SPECTRAL:
            self.post.nrs_select(rx)
        else:
            self.post.set_nr_algo(rx, algo)
        for t, vals in (params or {}).items():
            for k, v in enumerate(vals):
                self.post.set_nr_param(rx, t, k, v)
        for t in (post_mod.NR_DENOISE, post_mod.NR_AUTONOTCH):
            if enable[t]:
                self.post.set_nr_enable(rx, t, enable[t])

    def set_nb(self, rx, algo, params=None, enable=(0, 0), frate=None):
        """The noise-blanker commands for receiver rx as a client sends them (rx/rx_sound_cmd.cpp:454-501): `SET nb algo=`, then the
        blanker's parameters one at a time (params: [gate_usec, threshold]), then the enables (NB_BLANKER, NB_WF).  frate: the
        connection's audio rate (default: the bank's nominal one).  nb.NB_WILD (`SET nb algo=2`) goes through kg_rxbank_nbw_select;
        its params are [thresh, taps, impulse_samples] (post.NB_THRESH ..), every message runs nb_Wild_init, and enabling NB_BLANKER
        switches the Wild stage of the receiver's kg_post on: its audio then lags by taps + impulse_samples // 2 samples.  Call it
        after set_audio, whose connection start switches the stage off."""
        frate = self.fs if frate is None else frate
        if algo == nb_mod.NB_WILD:
            check(self.lib.kg_rxbank_nbw_select(self.h, int(rx)), "kg_rxbank_nbw_select")
        else:
            check(self.lib.kg_rxbank_set_nb_algo(self.h, int(rx), int(algo)), "kg_rxbank_set_nb_algo")
        for k, v in enumerate(params or []):
            check(self.lib.kg_rxbank_set_nb_param(self.h, int(rx), nb_mod.NB_BLANKER, k, float(np.float32(v)), float(np.float32(frate))),
                  "kg_rxbank_set_nb_param")
        for t in (nb_mod.NB_BLANKER, nb_mod.NB_WF):
            if enable[t]:
                check(self.lib.kg_rxbank_set_nb_enable(self.h, int(rx), t, int(enable[t])), "kg_rxbank_set_nb_enable")

    def set_nb_gate(self, rx, nb, th, frate=None):
        """kiwiclient's legacy `SET nb=<gate> th=<threshold>` (rx/rx_sound_cmd.cpp:660-672)."""
        frate = self.fs if frate is None else frate
        check(self.lib.kg_rxbank_set_nb_gate(self.h, int(rx), int(nb), int(th), float(np.float32(frate))), "kg_rxbank_set_nb_gate")

    def nb_cmd_state(self, rx):
        """-> (ints[14]: algo, snd enable[4], wf enable[4], wf nb_param_change[4], wf nb_setup; floats [2, 4, 8]: snd / wf nb_param)"""
        ints = np.zeros(14, np.int32)
        flts = np.zeros((2, 4, 8), np.float32)
        check(self.lib.kg_rxbank_nb_cmd_state(self.h, int(rx), ptr(ints), ptr(flts)), "kg_rxbank_nb_cmd_state")
        return ints, flts

    def set_spec(self, rx, n):
        """`SET spc_=n` (rx/rx_sound_cmd.cpp:332-339): 2 (SPEC_SND_AF) switches receiver rx's audio spectrum rows on, anything else
        off.  Call it after set_audio / join, whose connection start clears it."""
        check(self.lib.kg_rxbank_set_spec(self.h, int(rx), int(n)), "kg_rxbank_set_spec")

    def spec_map(self):
        """-> (rx_of_row, inst_of_row, blk_of_row) of the last step's audio spectrum rows, in emission order per receiver"""
        m = check(self.lib.kg_rxbank_spec_max(self.h), "kg_rxbank_spec_max")
        rx_of, inst, blk = (np.zeros(m, np.int32) for _ in range(3))
        n = check(self.lib.kg_rxbank_spec_map(self.h, ptr(rx_of), ptr(inst), ptr(blk)), "kg_rxbank_spec_map")
        return rx_of[:n], inst[:n], blk[:n]

    def spec_rows(self):
        """-> uint8 [rows, 1024]: the last step's audio spectrum rows (after sync()), row r described by spec_map()[.][r]"""
        n = check(self.lib.kg_rxbank_spec_map(self.h, None, None, None), "kg_rxbank_spec_map")
        d, stride = C.c_void_p(), C.c_size_t()
        check(self.lib.kg_rxbank_spec_rows(self.h, C.byref(d), C.byref(stride)), "kg_rxbank_spec_rows")
        out = np.zeros((n, int(stride.value)), np.uint8)
        if n:
            self.ctx.download(int(d.value), out)
        return out[:, :1024]

    # ---- the IQ display extension (extensions/IQ_display/iq_display.cpp): kg_iqd's commands per receiver
    def iqd_init(self, rx):
        check(self.lib.kg_rxbank_iqd_init(self.h, int(rx)), "kg_rxbank_iqd_init")

    def iqd_set_run(self, rx, run, rate):
        check(self.lib.kg_rxbank_iqd_set_run(self.h, int(rx), int(run), float(rate)), "kg_rxbank_iqd_set_run")

    def iqd_set_gain(self, rx, gain):
        check(self.lib.kg_rxbank_iqd_set_gain(self.h, int(rx), int(gain)), "kg_rxbank_iqd_set_gain")

    def iqd_set_points(self, rx, points):
        check(self.lib.kg_rxbank_iqd_set_points(self.h, int(rx), int(points)), "kg_rxbank_iqd_set_points")

    def iqd_set_pll_mode(self, rx, pll_mode, arg):
        check(self.lib.kg_rxbank_iqd_set_pll_mode(self.h, int(rx), int(pll_mode), int(arg)), "kg_rxbank_iqd_set_pll_mode")

    def iqd_set_pll_bandwidth(self, rx, bandwidth):
        check(self.lib.kg_rxbank_iqd_set_pll_bandwidth(self.h, int(rx), float(bandwidth)), "kg_rxbank_iqd_set_pll_bandwidth")

    def iqd_set_draw(self, rx, draw):
        check(self.lib.kg_rxbank_iqd_set_draw(self.h, int(rx), int(draw)), "kg_rxbank_iqd_set_draw")

    def iqd_set_display_mode(self, rx, display_mode):
        check(self.lib.kg_rxbank_iqd_set_display_mode(self.h, int(rx), int(display_mode)), "kg_rxbank_iqd_set_display_mode")

    def iqd_clear(self, rx):
        check(self.lib.kg_rxbank_iqd_clear(self.h, int(rx)), "kg_rxbank_iqd_clear")

    @property
    def iqd(self):
        """the bank's IqDisplay (None until one of the iqd_* commands was sent): state()"""
        from . import iqd as iq_mod
        h = self.lib.kg_rxbank_iqd(self.h)
        return borrow(iq_mod.IqDisplay, self.ctx, h, nchan=self.nrx) if h else None

    def iqd_rows(self):
        """-> (row map [rows] of iqd.row_dtype -- ch the receiver, blk the sound block of the step --, the rows' bytes uint8) of the
        last step (after sync())"""
        from . import iqd as iq_mod
        n = check(self.lib.kg_rxbank_iqd_map(self.h, None, 0), "kg_rxbank_iqd_map")
        m = np.zeros(max(n, 1), iq_mod.row_dtype)
        check(self.lib.kg_rxbank_iqd_map(self.h, ptr(m), int(m.size)), "kg_rxbank_iqd_map")
        m = m[:n]
        d, cap = C.c_void_p(), C.c_size_t()
        check(self.lib.kg_rxbank_iqd_rows(self.h, C.byref(d), C.byref(cap)), "kg_rxbank_iqd_rows")
        out = np.zeros(int(m["off"][-1] + m["len"][-1]) if n else 0, np.uint8)
        if out.size:
            self.ctx.download(int(d.value), out)
        return m, out

    def iqd_status(self):
        """-> (records of iqd.status_dtype, rx_of_blk, blk_of_blk, sent_of_blk) of the last step (after sync())"""
        from . import iqd as iq_mod
        n = check(self.lib.kg_rxbank_iqd_status(self.h, None, None, None, None), "kg_rxbank_iqd_status")
        rx_of, blk, sent = (np.zeros(max(n, 1), np.int32) for _ in range(3))
        d = C.c_void_p()
        check(self.lib.kg_rxbank_iqd_status(self.h, C.byref(d), ptr(rx_of), ptr(blk), ptr(sent)), "kg_rxbank_iqd_status")
        st = np.zeros(n, iq_mod.status_dtype)
        if n:
            self.ctx.download(int(d.value), st)
        return st, rx_of[:n], blk[:n], sent[:n]

    # ---- the Loran-C extension (extensions/Loran_C/loran_c.cpp): kg_lorc's commands per receiver
    def lorc_init(self, rx, srate, i_srate):
        check(self.lib.kg_rxbank_lorc_init(self.h, int(rx), float(srate), int(i_srate)), "kg_rxbank_lorc_init")

    def lorc_set_gri(self, rx, ch, gri):
        check(self.lib.kg_rxbank_lorc_set_gri(self.h, int(rx), int(ch), int(gri)), "kg_rxbank_lorc_set_gri")

    def lorc_set_offset(self, rx, ch, offset):
        check(self.lib.kg_rxbank_lorc_set_offset(self.h, int(rx), int(ch), int(offset)), "kg_rxbank_lorc_set_offset")

    def lorc_set_gain(self, rx, ch, gain):
        check(self.lib.kg_rxbank_lorc_set_gain(self.h, int(rx), int(ch), int(gain)), "kg_rxbank_lorc_set_gain")

    def lorc_set_avg_algo(self, rx, ch, avg_algo):
        check(self.lib.kg_rxbank_lorc_set_avg_algo(self.h, int(rx), int(ch), int(avg_algo)), "kg_rxbank_lorc_set_avg_algo")

    def lorc_set_avg_param(self, rx, ch, avg_param):
        check(self.lib.kg_rxbank_lorc_set_avg_param(self.h, int(rx), int(ch), float(avg_param)), "kg_rxbank_lorc_set_avg_param")

    def lorc_start(self, rx):
        check(self.lib.kg_rxbank_lorc_start(self.h, int(rx)), "kg_rxbank_lorc_start")

    def lorc_stop(self, rx):
        check(self.lib.kg_rxbank_lorc_stop(self.h, int(rx)), "kg_rxbank_lorc_stop")

    @property
    def lorc(self):
        """the bank's LoranC (None until one of the lorc_* commands was sent): state()"""
        from . import lorc as lo_mod
        h = self.lib.kg_rxbank_lorc(self.h)
        return borrow(lo_mod.LoranC, self.ctx, h, nconn=self.nrx) if h else None

    def lorc_rows(self):
        """-> (row map [rows] of lorc.row_dtype -- conn the receiver, blk the sound block of the step --, the rows' bytes uint8 from the
        buffer's start to the last row's end) of the last step (after sync())"""
        from . import lorc as lo_mod
        n = check(self.lib.kg_rxbank_lorc_map(self.h, None, 0), "kg_rxbank_lorc_map")
        m = np.zeros(max(n, 1), lo_mod.row_dtype)
        check(self.lib.kg_rxbank_lorc_map(self.h, ptr(m), int(m.size)), "kg_rxbank_lorc_map")
        m = m[:n]
        d, cap = C.c_void_p(), C.c_size_t()
        check(self.lib.kg_rxbank_lorc_rows(self.h, C.byref(d), C.byref(cap)), "kg_rxbank_lorc_rows")
        out = np.zeros(int(m["off"][-1] + m["len"][-1]) if n else 0, np.uint8)
        if out.size:
            self.ctx.download(int(d.value), out)
        return m, out

    # ---- the FAX extension (extensions/FAX/FaxDecoder.cpp, fax.cpp): kg_fax's commands per receiver
    def fax_start(self, rx, lpm=120, imagewidth=1024, carrier=1900, deviation=400, bandwidth=1, include_headers=True, phasing=True, autostop=True, debug=0,
                  nom_rate=12000.0, srate=None):
        """`SET fax_start` (the defaults are what fax.cpp:131-145 passes); srate stays the receiver's sample rate until the next start"""
        check(self.lib.kg_rxbank_fax_start(self.h, int(rx), int(lpm), int(imagewidth), int(carrier), int(deviation), int(bandwidth), int(bool(include_headers)),
                                           int(bool(phasing)), int(bool(autostop)), int(debug), float(nom_rate), float(nom_rate if srate is None else srate)),
              "kg_rxbank_fax_start")

    def fax_set_shift(self, rx, shift):
        check(self.lib.kg_rxbank_fax_set_shift(self.h, int(rx), float(shift)), "kg_rxbank_fax_set_shift")

    def fax_stop(self, rx):
        check(self.lib.kg_rxbank_fax_stop(self.h, int(rx)), "kg_rxbank_fax_stop")

    @property
    def fax(self):
        """the bank's FaxDecoder (None until one of the fax_* commands was sent): state()"""
        from . import fax as fa_mod
        h = self.lib.kg_rxbank_fax(self.h)
        return borrow(fa_mod.FaxDecoder, self.ctx, h, nconn=self.nrx) if h else None

    def fax_out(self):
        """-> {receiver: (records of fax.rec_dtype -- blk the sound block of the step --, rows uint8 [rows, row_stride])} of the last step
        (after sync()): the receivers the step fed"""
        from . import fax as fa_mod
        rxs = np.zeros(self.nrx, np.int32)
        d_rows, stride, d_recs, d_counts, ml = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_void_p(), C.c_int32()
        n = check(self.lib.kg_rxbank_fax_out(self.h, C.byref(d_rows), C.byref(stride), C.byref(d_recs), C.byref(d_counts), C.byref(ml), ptr(rxs), int(rxs.size)),
                  "kg_rxbank_fax_out")
        out = {}
        if n == 0:
            return out
        counts = np.zeros((n, 4), np.int32)
        self.ctx.download(int(d_counts.value), counts)
        assert not counts[:, 2].any(), "a capacity was exceeded"
        for e in range(n):
            recs = np.zeros(int(counts[e, 1]), fa_mod.rec_dtype)
            rows = np.zeros((int(counts[e, 0]), int(stride.value)), np.uint8)
            if recs.size:
                self.ctx.download(int(d_recs.value) + e * ml.value * fa_mod.rec_dtype.itemsize, recs)
            if rows.size:
                self.ctx.download(int(d_rows.value) + e * ml.value * int(stride.value), rows)
            out[int(rxs[e])] = (recs, rows)
        return out

    # ---- the CW decoder extension (extensions/CW_decoder/uhsdr_cw_decoder.cpp, cw_decoder.cpp): kg_cw's commands per receiver
    def cw_start(self, rx, training_interval=100, nom_rate=12000.0, srate=None):
        """`SET cw_start=` / `SET cw_train=`; refused while FAX is started on the receiver (the real-samples tap holds one task)"""
        check(self.lib.kg_rxbank_cw_start(self.h, int(rx), int(training_interval), float(nom_rate), float(nom_rate if srate is None else srate)),
              "kg_rxbank_cw_start")

    def cw_set_wpm(self, rx, wpm, training_interval=100):
        check(self.lib.kg_rxbank_cw_set_wpm(self.h, int(rx), int(wpm), int(training_interval)), "kg_rxbank_cw_set_wpm")
        return "EXT cw_train=0" if int(wpm) != 0 else None

    def cw_set_pboff(self, rx, pboff):
        check(self.lib.kg_rxbank_cw_set_pboff(self.h, int(rx), int(pboff) & 0xffffffff), "kg_rxbank_cw_set_pboff")

    def cw_set_wsc(self, rx, wsc):
        check(self.lib.kg_rxbank_cw_set_wsc(self.h, int(rx), int(wsc)), "kg_rxbank_cw_set_wsc")

    def cw_set_auto_threshold(self, rx, on):
        check(self.lib.kg_rxbank_cw_set_auto_threshold(self.h, int(rx), int(on)), "kg_rxbank_cw_set_auto_threshold")

    def cw_set_threshold(self, rx, threshold):
        check(self.lib.kg_rxbank_cw_set_threshold(self.h, int(rx), int(threshold)), "kg_rxbank_cw_set_threshold")

    def cw_stop(self, rx):
        check(self.lib.kg_rxbank_cw_stop(self.h, int(rx)), "kg_rxbank_cw_stop")

    def cw_set_now(self, now_sec):
        """what timer_sec() answers during every later step"""
        check(self.lib.kg_rxbank_cw_set_now(self.h, int(now_sec) & 0xffffffff), "kg_rxbank_cw_set_now")

    # ---- the WSPR extension, stage 1 (extensions/wspr/wspr_main.cpp, wspr.cpp): kg_wspr's commands per receiver
    def wspr_init(self, rx, snd_rate=12000.0):
        """`SET ext_server_init`; int_decimate = (int) (snd_rate / 375.0)"""
        check(self.lib.kg_rxbank_wspr_init(self.h, int(rx), float(snd_rate)), "kg_rxbank_wspr_init")

    def wspr_set_capture(self, rx, capture):
        """`SET capture=`; on, refused while the IQ display runs or Loran-C is started on the receiver (the IQ tap holds one callback)"""
        check(self.lib.kg_rxbank_wspr_set_capture(self.h, int(rx), int(capture)), "kg_rxbank_wspr_set_capture")

    def wspr_set_type(self, rx, wspr_type):
        check(self.lib.kg_rxbank_wspr_set_type(self.h, int(rx), int(wspr_type)), "kg_rxbank_wspr_set_type")

    def wspr_set_more_candidates(self, rx, on):
        check(self.lib.kg_rxbank_wspr_set_more_candidates(self.h, int(rx), int(on)), "kg_rxbank_wspr_set_more_candidates")

    def wspr_set_now(self, minute, second):
        """what utc_hour_min_sec answers during every later step"""
        check(self.lib.kg_rxbank_wspr_set_now(self.h, int(minute), int(second)), "kg_rxbank_wspr_set_now")

    def wspr_set_metric_table(self, mettab):
        """stage 2: mettab int32 [2, 256] for the bank's Wspr"""
        mt = np.ascontiguousarray(mettab, np.int32)
        assert mt.shape == (2, 256)
        check(self.lib.kg_rxbank_wspr_set_metric_table(self.h, ptr(mt)), "kg_rxbank_wspr_set_metric_table")

    def wspr_set_decode(self, rx, on):
        """on: a step that holds the receiver's cycle end also enqueues pass 0 (200, 2) behind it"""
        check(self.lib.kg_rxbank_wspr_set_decode(self.h, int(rx), int(on)), "kg_rxbank_wspr_set_decode")

    def wspr_dec_out(self):
        """-> ({receiver: records of wspr.dec_dtype} of the receivers whose pass 0 the last step enqueued; after sync())"""
        from . import wspr as ws
        rxs = np.zeros(self.nrx, np.int32)
        d_decs, d_n = C.c_void_p(), C.c_void_p()
        n = check(self.lib.kg_rxbank_wspr_dec_out(self.h, C.byref(d_decs), C.byref(d_n), ptr(rxs), int(rxs.size)), "kg_rxbank_wspr_dec_out")
        out = {}
        if n:
            recs, cnt = np.zeros((self.nrx, ws.MAX_NPK), ws.dec_dtype), np.zeros(self.nrx, np.int32)
            self.ctx.download(int(d_decs.value), recs)
            self.ctx.download(int(d_n.value), cnt)
            for rx in rxs[:n].tolist():
                out[rx] = recs[rx][:cnt[rx]].copy()
        return out

    @property
    def wspr(self):
        """the bank's Wspr (None until one of the per-receiver wspr_* commands was sent): state()"""
        from . import wspr as ws
        h = self.lib.kg_rxbank_wspr(self.h)
        return borrow(ws.Wspr, self.ctx, h, nconn=self.nrx) if h else None

    def wspr_out(self):
        """-> (rows [n, 412] uint8, row map of wspr.row_dtype -- conn the receiver, blk the sound block of the step --, events of
        wspr.ev_dtype, {receiver: cycle record} of the receivers whose cycle ended, {receiver: counts [4]}) of the last step (after sync())"""
        from . import wspr as ws
        m, ev, rxs = np.zeros(self.nrx * 256, ws.row_dtype), np.zeros(self.nrx * 16, ws.ev_dtype), np.zeros(self.nrx, np.int32)
        d_rows, d_cyc, d_cnt, n, ne = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int32(), C.c_int32()
        nent = check(self.lib.kg_rxbank_wspr_out(self.h, C.byref(d_rows), C.byref(d_cyc), C.byref(d_cnt), ptr(m), int(m.size), C.byref(n), ptr(ev), int(ev.size),
                                                 C.byref(ne), ptr(rxs), int(rxs.size)), "kg_rxbank_wspr_out")
        rows = np.zeros((n.value, ws.NBINS + 1), np.uint8)
        cycles, counts = {}, {}
        if nent:
            cy, cn = np.zeros(nent, ws.cycle_dtype), np.zeros((nent, 4), np.int32)
            self.ctx.download(int(d_cyc.value), cy)
            self.ctx.download(int(d_cnt.value), cn)
            for e in range(nent):
                counts[int(rxs[e])] = cn[e].copy()
                if cy[e]["due"]:
                    cycles[int(rxs[e])] = cy[e].copy()
        if n.value:
            slots = np.zeros((n.value, ws.ROW_STRIDE), np.uint8)
            self.ctx.download(int(d_rows.value), slots)
            assert not slots[:, ws.NBINS + 1:].any()
            rows[:] = slots[:, :ws.NBINS + 1]
        return rows, m[:n.value].copy(), ev[:ne.value].copy(), cycles, counts

    # ---- the FT8 / FT4 extension, stage 1 (extensions/FT8/ft8_lib): kg_ft8's commands per receiver
    def ft8_init(self, rx, protocol=0, snd_rate=12000.0):
        """decode_ft8_init / decode_ft8_protocol: the receiver's connection begins again"""
        check(self.lib.kg_rxbank_ft8_init(self.h, int(rx), int(protocol), float(snd_rate)), "kg_rxbank_ft8_init")

    def ft8_start(self, rx):
        """registers the real-samples task; refused while FAX or the CW decoder is started on the receiver (the tap holds one task)"""
        check(self.lib.kg_rxbank_ft8_start(self.h, int(rx)), "kg_rxbank_ft8_start")

    def ft8_stop(self, rx):
        check(self.lib.kg_rxbank_ft8_stop(self.h, int(rx)), "kg_rxbank_ft8_stop")

    def ft8_set_now(self, now):
        """what clock_gettime answers, in seconds, during every later step"""
        check(self.lib.kg_rxbank_ft8_set_now(self.h, float(now)), "kg_rxbank_ft8_set_now")

    @property
    def ft8(self):
        """the bank's Ft8 (None until one of the per-receiver ft8_* commands was sent): state(), set_snr_adj()"""
        from . import ft8 as f8
        h = self.lib.kg_rxbank_ft8(self.h)
        return borrow(f8.Ft8, self.ctx, h, nconn=self.nrx) if h else None

    def ft8_out(self):
        """-> (events of ft8.ev_dtype -- conn the receiver, cb the sound block of the step --, {receiver: slot record of ft8.slot_dtype} of
        the receivers whose slot ended) of the last step (after sync())"""
        from . import ft8 as f8
        ev, rxs = np.zeros(self.nrx * 4, f8.ev_dtype), np.zeros(self.nrx, np.int32)
        d_slots, ne = C.c_void_p(), C.c_int32()
        n = check(self.lib.kg_rxbank_ft8_out(self.h, C.byref(d_slots), ptr(ev), int(ev.size), C.byref(ne), ptr(rxs), int(rxs.size)), "kg_rxbank_ft8_out")
        slots = {}
        if n:
            recs = np.zeros(n, f8.slot_dtype)
            self.ctx.download(int(d_slots.value), recs)
            for k in range(n):
                assert recs[k]["due"] == 1 and recs[k]["conn"] == rxs[k]
                slots[int(rxs[k])] = recs[k].copy()
        return ev[:ne.value].copy(), slots

    @property
    def cw(self):
        """the bank's CwDecoder (None until one of the per-receiver cw_* commands was sent): state()"""
        from . import cw as cw_mod
        h = self.lib.kg_rxbank_cw(self.h)
        return borrow(cw_mod.CwDecoder, self.ctx, h, nconn=self.nrx) if h else None

    def cw_out(self):
        """-> {receiver: events of cw.ev_dtype -- blk the sound block of the step --} of the last step (after sync()): the receivers the
        step fed"""
        from . import cw as cw_mod
        rxs = np.zeros(self.nrx, np.int32)
        d_evs, d_counts, me = C.c_void_p(), C.c_void_p(), C.c_int32()
        n = check(self.lib.kg_rxbank_cw_out(self.h, C.byref(d_evs), C.byref(d_counts), C.byref(me), ptr(rxs), int(rxs.size)), "kg_rxbank_cw_out")
        out = {}
        if n == 0:
            return out
        counts = np.zeros((n, 4), np.int32)
        self.ctx.download(int(d_counts.value), counts)
        assert not counts[:, 2].any(), "the event capacity was exceeded"
        for e in range(n):
            evs = np.zeros(int(counts[e, 0]), cw_mod.ev_dtype)
            if evs.size:
                self.ctx.download(int(d_evs.value) + e * me.value * cw_mod.ev_dtype.itemsize, evs)
            out[int(rxs[e])] = evs
        return out

    def fftext_set_rate(self, sample_rate):
        """what ext_update_get_sample_rateHz answers for the FFT extension (extensions/FFT/FFT.cpp:79)"""
        check(self.lib.kg_rxbank_fftext_set_rate(self.h, float(sample_rate)), "kg_rxbank_fftext_set_rate")

    def fftext_set_run(self, rx, run):
        """`SET run=%d` of the FFT extension (fftext.OFF / WF / SPEC / INTEG); isSAM and QAM are read from receiver rx's mode now"""
        check(self.lib.kg_rxbank_fftext_set_run(self.h, int(rx), int(run)), "kg_rxbank_fftext_set_run")

    def fftext_set_itime(self, rx, itime):
        check(self.lib.kg_rxbank_fftext_set_itime(self.h, int(rx), float(itime)), "kg_rxbank_fftext_set_itime")

    def fftext_clear(self, rx):
        check(self.lib.kg_rxbank_fftext_clear(self.h, int(rx)), "kg_rxbank_fftext_clear")

    @property
    def fftext(self):
        """the bank's FftExt (None until one of the fftext_* commands was sent): due(), state()"""
        from . import fftext as fx_mod
        h = self.lib.kg_rxbank_fftext(self.h)
        return borrow(fx_mod.FftExt, self.ctx, h, nchan=self.nrx) if h else None

    def fftext_map(self):
        """-> (rx_of_row, blk_of_row, bin_of_row) of the last step's extension rows, per receiver in block order"""
        m = check(self.lib.kg_rxbank_fftext_max(self.h), "kg_rxbank_fftext_max")
        rx_of, blk, bins = (np.zeros(m, np.int32) for _ in range(3))
        n = check(self.lib.kg_rxbank_fftext_map(self.h, ptr(rx_of), ptr(blk), ptr(bins)), "kg_rxbank_fftext_map")
        return rx_of[:n], blk[:n], bins[:n]

    def fftext_rows(self):
        """-> uint8 [rows, 1024]: the last step's extension rows (after sync()), row r described by fftext_map()[.][r]"""
        n = check(self.lib.kg_rxbank_fftext_map(self.h, None, None, None), "kg_rxbank_fftext_map")
        d, stride = C.c_void_p(), C.c_size_t()
        check(self.lib.kg_rxbank_fftext_rows(self.h, C.byref(d), C.byref(stride)), "kg_rxbank_fftext_rows")
        out = np.zeros((n, int(stride.value)), np.uint8)
        if n:
            self.ctx.download(int(d.value), out)
        return out[:, :1024]

    def set_little_endian(self, rx, little_endian):
        check(self.lib.kg_rxbank_set_little_endian(self.h, int(rx), int(bool(little_endian))), "kg_rxbank_set_little_endian")
        self.little_endian[rx] = bool(little_endian)

    def leave(self, rx):
        check(self.lib.kg_rxbank_leave(self.h, int(rx)), "kg_rxbank_leave")

    def is_active(self, rx):
        return check(self.lib.kg_rxbank_is_active(self.h, int(rx)), "kg_rxbank_is_active") == 1

    def audio_map(self):
        """-> (nrec, nfir, fir_pos, snd_seq) per receiver after the last step"""
        nrec, nfir, pos = (np.zeros(self.nrx, np.int32) for _ in range(3))
        seq = np.zeros(self.nrx, np.uint32)
        check(self.lib.kg_rxbank_audio_map(self.h, ptr(nrec), ptr(nfir), ptr(pos), ptr(seq)), "kg_rxbank_audio_map")
        return nrec, nfir, pos, seq

    def ready(self):
        """False: the next step() would wait for its table slot (the host is KG_RXBANK_SLOTS steps ahead of the GPU)."""
        return check(self.lib.kg_rxbank_ready(self.h), "kg_rxbank_ready") == 1

    # ---- the step
    def step(self, d_adc, adc_ready_event=None):
        """One step over n ADC samples at d_adc (device pointer, int).  Enqueue only.  -> StepInfoC"""
        info = StepInfoC()
        check(self.lib.kg_rxbank_step(self.h, ptr(int(d_adc)), ptr(int(adc_ready_event)) if adc_ready_event else None,
                                      C.byref(info)), "kg_rxbank_step")
        return info

    def step_fast(self, d_adc):
        """step() without the info structure: the timed loop."""
        check(self.lib.kg_rxbank_step(self.h, C.c_void_p(d_adc), None, None), "kg_rxbank_step")

    def sync(self):
        check(self.lib.kg_rxbank_sync(self.h), "kg_rxbank_sync")

    def poll(self):
        return check(self.lib.kg_rxbank_poll(self.h), "kg_rxbank_poll") == 1

    def adc_done(self, stream, steps_back=1):
        """`stream` waits for the readers of the ADC block of the step `steps_back` steps ago (2: the buffer a double-buffered
        ring refills next)."""
        check(self.lib.kg_rxbank_adc_done(self.h, C.c_void_p(int(stream)), int(steps_back)), "kg_rxbank_adc_done")

    def host_profile(self):
        """Where the host's share of the steps since the last call went (text; kg_rxbank_host_profile)."""
        buf = C.create_string_buffer(1024)
        check(self.lib.kg_rxbank_host_profile(self.h, buf, 1024), "kg_rxbank_host_profile")
        return buf.value.decode()

    def frame_map(self):
        """-> (rx_of_frame, frame_off, pkt_bytes) of the last step"""
        rx_of = np.zeros(self.nrx, np.int32)
        off = np.zeros(self.nrx, np.uint64)
        nb = np.zeros(self.nrx, np.int32)
        nf = check(self.lib.kg_rxbank_frame_map(self.h, ptr(rx_of), ptr(off), ptr(nb)), "kg_rxbank_frame_map")
        return rx_of[:nf], off[:nf], nb[:nf]

    # ---- results to the host (after sync())
    def _rows(self, dptr, row_bytes, rows, dtype, shape_tail):
        """rows `rows` (a list of indices) of a [*, row_bytes] device array -> numpy [len(rows), ...]"""
        out = np.zeros((len(rows), row_bytes), np.uint8)
        for i, r in enumerate(rows):
            self.ctx.download(dptr + int(r) * row_bytes, out[i])
        return out.view(dtype).reshape((len(rows),) + shape_tail)

    def fetch(self, what, rows):
        b = self.bufs
        if what == "wf_iq":
            return self._rows(b.wf_iq, b.wf_iq_stride * 4, rows, np.int16, (b.wf_iq_stride, 2))
        if what == "rows":
            return self._rows(b.wf_rows, 1024, rows, np.uint8, (1024,))
        if what == "pkts":
            return self._rows(b.wf_pkts, b.wf_pkt_stride, rows, np.uint8, (b.wf_pkt_stride,))
        if what == "raw":
            return self._rows(b.rx_raw, b.rx_stride * 6, rows, np.uint8, (b.rx_stride * 6,))
        if what == "xin":
            return self._rows(b.rx_in, b.rx_stride * 8, rows, np.float32, (b.rx_stride, 2))
        if what == "firo":
            return self._rows(b.fir_out, b.fir_stride * 8, rows, np.float32, (b.fir_stride, 2))
        if what == "s16":
            return self._rows(b.s16, b.fir_stride * 2, rows, np.int16, (b.fir_stride,))
        if what == "pay":
            return self._rows(b.adpcm, b.fir_stride // 2, rows, np.uint8, (b.fir_stride // 2,))
        if what == "agc":
            return self._rows(b.agc, b.fir_stride * 8, rows, np.float32, (b.fir_stride, 2))
        if what == "iq_pay":
            return self._rows(b.iq_pay, b.fir_stride * 4, rows, np.uint8, (b.fir_stride * 4,))
        raise KeyError(what)
