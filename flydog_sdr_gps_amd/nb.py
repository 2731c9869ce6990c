"""Host-side mirror of the reference's standard noise blanker (NB_STD) over the C ABI (kg_nb, include/kiwigpu.h).

Reference (rx/CuteSDR/noiseproc.cpp, CNoiseProc)          here
  m_NoiseProc_snd[]                  rx/rx_sound.cpp     ->  NoiseBlanker (one blanker per channel)
  SetupBlanker(id, rate, nb_param)   :89-145             ->  NoiseBlanker.setup()
  ProcessBlanker(n, in, out)         :147-203            ->  NoiseBlanker.process() / process_dev()  (GPU, libkiwigpu.so)
The waterfall's blankers (m_NoiseProc_wf[]) belong to the Waterfall object (Waterfall.nb_setup / set_nb / nb_frames / nb_state).
"""
import ctypes as C

import numpy as np

from ._lib import Context, check, ptr

NB_OFF, NB_STD, NB_WILD = 0, 1, 2                 # nb_algo_e, rx/rx_noise.h:6
NB_BLANKER, NB_WF, NB_CLICK = 0, 1, 2             # nb_type_e, rx/rx_noise.h:7
NB_GATE, NB_THRESHOLD = 0, 1                      # extensions/noise_blank/noise_blank.h
NB_PARAMS = 8                                     # NOISE_PARAMS, rx/rx_noise.h:4
MAG_CAP = 1024                                    # KG_NB_MAG_CAP: the largest 0.005 x sample rate a setup accepts


class NoiseBlanker:
    """GPU noise blankers for nchan channels on one device (kg_nb)."""

    def __init__(self, ctx=None, nchan=4, max_in=4096, device=0):
        self.ctx = ctx if ctx is not None else Context(device)
        self.lib = self.ctx.lib
        self.nchan, self.max_in = nchan, max_in
        h = C.c_void_p()
        check(self.lib.kg_nb_create(self.ctx.h, int(nchan), int(max_in), C.byref(h)), "kg_nb_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None) and not getattr(self, "_borrowed", False):
                self.lib.kg_nb_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def setup(self, ch, sample_rate, params):
        """SetupBlanker("SND", sample_rate, params): params = [gate_usec, threshold, ...] (up to 8 values)."""
        p = np.zeros(NB_PARAMS, np.float32)
        p[:len(params)] = params
        check(self.lib.kg_nb_setup(self.h, int(ch), float(np.float32(sample_rate)), ptr(p)), "kg_nb_setup")

    def process(self, ch, x):
        """ProcessBlanker on complex floats [n, 2] (host, synchronous) -> [n, 2] float32."""
        x = np.ascontiguousarray(x, np.float32).reshape(-1, 2)
        out = np.empty_like(x)
        check(self.lib.kg_nb_process(self.h, int(ch), ptr(x), x.shape[0], ptr(out)), "kg_nb_process")
        return out

    def process_dev(self, chans, d_in, in_stride, counts, d_out, out_stride):
        """Device pointers (ints); strides in complex samples; enqueue only."""
        chans = np.ascontiguousarray(chans, np.int32)
        counts = np.ascontiguousarray(counts, np.int32)
        if counts.size != chans.size:
            raise ValueError("counts and chans differ in length")
        check(self.lib.kg_nb_process_dev(self.h, ptr(chans), chans.size, ptr(int(d_in)), int(in_stride), ptr(counts),
                                         ptr(int(d_out)), int(out_stride)), "kg_nb_process_dev")

    def state(self, chans):
        """-> (ints [n, 6]: m_Mptr, m_Dptr, m_BlankCounter, m_MagSamples, m_DelaySamples, m_GateSamples; floats [n, 2]: m_Ratio,
        m_MagAveSum)"""
        chans = np.ascontiguousarray(np.atleast_1d(chans), np.int32)
        ints = np.empty((chans.size, 6), np.int32)
        flts = np.empty((chans.size, 2), np.float32)
        check(self.lib.kg_nb_state(self.h, ptr(chans), chans.size, ptr(ints), ptr(flts)), "kg_nb_state")
        return ints, flts
