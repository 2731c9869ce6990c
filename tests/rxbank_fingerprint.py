"""One scenario of the receiver bank and everything a step of it hands out, as integers and digests: what
tools/make_rxbank_fingerprint_golden.py records into tests/golden/rxbank_fingerprint.npz and test_rxbank_fingerprint_gpu.py runs again.

Six receivers at n = 2^21 over two alternating ADC blocks.  Zooms 10 and 11 (R = 512 and 1024: 8192 R > n) are overlapped; R = 512 writes
4096 pairs a step into its ring of 65536, so the ring wraps on step 16 -- the seventeenth -- and the scenario runs eighteen steps.  201.3
records a step: a connection completes a 512-sample sound block every 2.54 steps, the one that joined on step 8 on steps of its own.

  rx  zoom  mode                          with
  0   8     AM, de-emphasis               NB_STD; `SET mod=` to SSB before step 11
  1   10    SSB                           `SET spc_=2`, NB_WILD
  2   9     NBFM, squelch
  3   11    SAM, channel null (LSB)       `SET spc_=2`, the FFT extension's spectrum (chosen in SAM: the second filter)
  4   8     IQ, little-endian             the FFT extension's waterfall
  5   9     QAM, big-endian               leaves before step 5, joins again before step 8
"""
import hashlib

import numpy as np

N, NRX, STEPS = 1 << 21, 6, 18
ZOOMS = [8, 10, 9, 11, 8, 9]
INFO_FIELDS = ("step", "nframes", "nrec", "nfir", "fir_pos", "snd_seq", "table_bytes", "nmoves")
BUFFERS = ("s16", "adpcm", "iq_pay", "wf_pkts", "spec_rows", "fftext_rows")
MUST_HOLD = ("s16", "adpcm", "wf_pkts")            # the integer paths, pinned bit-exact elsewhere: never left out of the fixture


def _audio():
    from flydog_sdr_gps_amd import post
    return {0: dict(lo=-2500.0, hi=2500.0, mode=post.MODE_AM, de_emp=1),
            1: dict(lo=300.0, hi=2700.0, mode=post.MODE_SSB),
            2: dict(lo=-3000.0, hi=3000.0, mode=post.MODE_NBFM, squelch=80),
            3: dict(lo=-4900.0, hi=4900.0, mode=post.MODE_SAM, sam_mparam=post.CHAN_NULL_LSB),
            4: dict(lo=-4900.0, hi=4900.0, mode=post.MODE_IQ),
            5: dict(lo=-4900.0, hi=4900.0, mode=post.MODE_QAM)}


def _sha(parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(np.ascontiguousarray(p).tobytes())
    return h.hexdigest()


def run():
    """-> {"info" [STEPS, 8], "audio_map" [STEPS, 4, NRX], "frame_n" / "frame_map" [STEPS, 3, NRX], "spec_n" / "spec_map", "fftext_n" /
    "fftext_map" (padded with -1), "digest_<buffer>" [STEPS] hex} of one run on the library that is loaded"""
    from flydog_sdr_gps_amd import fftext, nb, post, synth
    from flydog_sdr_gps_amd.ddc import rx_phase_inc
    from flydog_sdr_gps_amd.rxbank import ADC_CLOCK, UI_SRATE, RxBank
    from flydog_sdr_gps_amd.wf import WfParams
    hz = UI_SRATE / (1024 << 14)
    audio = _audio()
    mix = []
    for k, zoom in enumerate(ZOOMS):
        span = UI_SRATE / (1 << zoom)
        p = WfParams.for_zoom(zoom, (0.0123 * ADC_CLOCK - span * (0.2 + 0.07 * k)) / hz, adc_clock=ADC_CLOCK, ui_srate=UI_SRATE)
        mix.append((p, 8192 * p.decim > N, rx_phase_inc(0.0123 * ADC_CLOCK - 900.0 - 35.0 * k, ADC_CLOCK)))
    assert [ov for _, ov, _ in mix] == [False, True, False, True, False, False]
    stereo = {rx: audio[rx]["mode"] in (post.MODE_IQ, post.MODE_SAS, post.MODE_QAM) for rx in range(NRX)}
    adc = synth.adc_stream(2 * N, 0x5EED00F1)
    bank = RxBank(NRX, N)
    d_adc = bank.ctx.alloc(adc.nbytes)
    try:
        bank.ctx.upload(d_adc, adc)
        bank.wf.set_tables()
        for rx, (p, ov, inc) in enumerate(mix):
            bank.set_wf(rx, p, ov)
            bank.set_audio(rx, inc, **audio[rx])
        bank.set_little_endian(4, True)
        bank.set_nb(0, nb.NB_STD, [100.0, 50.0], (1, 1))
        bank.set_nb(1, nb.NB_WILD, [0.95, 10, 7], (1, 0))
        bank.set_spec(1, 2)
        bank.set_spec(3, 2)
        bank.fftext_set_rate(bank.fs)
        bank.fftext_set_run(3, fftext.SPEC)
        bank.fftext_set_run(4, fftext.WF)
        spec_max = int(bank.lib.kg_rxbank_spec_max(bank.h))
        fx_max = int(bank.lib.kg_rxbank_fftext_max(bank.h))
        out = {"info": np.zeros((STEPS, len(INFO_FIELDS)), np.int64), "audio_map": np.zeros((STEPS, 4, NRX), np.int64),
               "frame_n": np.zeros(STEPS, np.int64), "frame_map": np.full((STEPS, 3, NRX), -1, np.int64),
               "spec_n": np.zeros(STEPS, np.int64), "spec_map": np.full((STEPS, 3, spec_max), -1, np.int64),
               "fftext_n": np.zeros(STEPS, np.int64), "fftext_map": np.full((STEPS, 3, fx_max), -1, np.int64)}
        digests = {k: [] for k in BUFFERS}
        for step in range(STEPS):
            if step == 5:
                bank.leave(5)
            if step == 8:
                bank.join(5, (mix[5][0], mix[5][1]), mix[5][2], **audio[5])
            if step == 11:                                              # `SET mod=` on a running connection
                bank.set_audio(0, mix[0][2], lo=300.0, hi=2700.0, mode=post.MODE_SSB)
            info = bank.step(d_adc + 2 * (step % 2) * N)
            bank.sync()
            out["info"][step] = [int(getattr(info, f)) for f in INFO_FIELDS]
            amap = bank.audio_map()
            out["audio_map"][step] = np.array([np.asarray(a, np.int64) for a in amap])
            for name, maps in (("frame", bank.frame_map()), ("spec", bank.spec_map()), ("fftext", bank.fftext_map())):
                n = len(maps[0])
                out[name + "_n"][step] = n
                for j, m in enumerate(maps):
                    out[name + "_map"][step, j, :n] = np.asarray(m).astype(np.int64)
            # the written extent of every buffer, from the maps
            nfir = [int(v) for v in amap[1]]
            real = [rx for rx in range(NRX) if nfir[rx] and not stereo[rx]]
            pairs = [rx for rx in range(NRX) if nfir[rx] and stereo[rx]]
            pkt_bytes = bank.frame_map()[2]
            s16, pay, iqp = bank.fetch("s16", real), bank.fetch("pay", real), bank.fetch("iq_pay", pairs)
            pkts = bank.fetch("pkts", list(range(len(pkt_bytes))))
            digests["s16"].append(_sha(s16[i, :nfir[rx]] for i, rx in enumerate(real)))
            digests["adpcm"].append(_sha(pay[i, :nfir[rx] // 2] for i, rx in enumerate(real)))
            digests["iq_pay"].append(_sha(iqp[i, :4 * nfir[rx]] for i, rx in enumerate(pairs)))
            digests["wf_pkts"].append(_sha(pkts[f, :int(nb_)] for f, nb_ in enumerate(pkt_bytes)))
            digests["spec_rows"].append(_sha([bank.spec_rows()]))
            digests["fftext_rows"].append(_sha([bank.fftext_rows()]))
        for k, v in digests.items():
            out["digest_" + k] = np.array(v)
        return out
    finally:
        bank.sync()
        bank.ctx.free(d_adc)
        bank.close()


def check_preconditions(out):
    """the scenario reaches what it is there for"""
    info = out["info"]
    assert (info[:, INFO_FIELDS.index("nmoves")] > 0).any(), "no ring wrapped"
    # sound blocks complete on different steps for different receivers: two steps whose block lists differ, one of them not everybody's
    lists = {tuple(np.flatnonzero(out["audio_map"][s, 1] > 0)) for s in range(STEPS)} - {()}
    assert len(lists) >= 2, lists
    assert any((out["spec_map"][s, 1, :out["spec_n"][s]] == 1).any() for s in range(STEPS)), "no channel-null row"
    assert (out["fftext_n"] > 0).any(), "no extension row"
    assert (out["spec_map"][:, 1, :] == 0).any(), "no passband row"
    assert any(out["frame_n"][s] < NRX for s in range(STEPS)) and out["frame_n"].max() == NRX
