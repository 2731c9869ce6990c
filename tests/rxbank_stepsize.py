"""One ADC stream through a receiver bank at a step size of the caller's choice, and everything the steps hand out, collected per
receiver as STREAMS: what test_rxbank_stepsize_gpu.py runs twice -- a long-step bank (several 512-sample sound blocks per receiver in one
kg_rxbank_step) and a short-step bank over the same samples with the same commands at the same sample positions -- and compares byte for
byte.  Behind the DDC the audio side is a stream machine (the bank section): how the stream is cut into steps must not show.

A scenario is a table, one row per receiver:
  zoom     waterfall zoom (a one-shot frame at every step size used)
  audio    RxBank.set_audio's keyword arguments
  le       `SET little-endian`
  nb       (algo, params, (NB_BLANKER, NB_WF)) for RxBank.set_nb
  spec     `SET spc_=`
  nr       (algo, params, (denoise, auto-notch)) for RxBank.set_nr
  fx       (run, itime or None): the FFT extension's `SET itime=` / `SET run=`, sent after the mode is set
A script maps a SAMPLE POSITION of the stream to commands sent before the step that starts there: (rx, what, value) with what in
"audio" (set_audio keywords: `SET mod=` on a running connection), "nr" (an nr triple), "leave", "join" (the row's whole configuration
again, as a new connection's first commands), "fx_clear".
"""
import functools

import numpy as np

SEED = 0x5EED0515
BLOCK = 1 << 24
STREAMS = ("raw", "xin", "firo", "agc", "s16", "pay", "iq_pay")        # the order a difference is looked for: the first stage that differs is the bug's
INFO_FIELDS = ("step", "nframes", "nrec", "nfir", "fir_pos", "snd_seq", "table_bytes", "nmoves")


def features():
    """(a): every feature of the bank; zooms 8..10 are one-shot frames at n = 2^22 and at 2^24"""
    from flydog_sdr_gps_amd import fftext, nb, post
    wide = dict(lo=-4900.0, hi=4900.0)
    return [dict(zoom=8, audio=dict(lo=-2500.0, hi=2500.0, mode=post.MODE_AM, de_emp=1), nb=(nb.NB_STD, [100.0, 50.0], (1, 1))),
            dict(zoom=10, audio=dict(lo=300.0, hi=2700.0, mode=post.MODE_SSB), spec=2, nb=(nb.NB_WILD, [0.95, 10, 7], (1, 0))),
            dict(zoom=9, audio=dict(lo=-3000.0, hi=3000.0, mode=post.MODE_NBFM, squelch=80)),
            dict(zoom=10, audio=dict(mode=post.MODE_SAM, sam_mparam=post.CHAN_NULL_LSB, **wide), spec=2, fx=(fftext.SPEC, None)),
            dict(zoom=8, audio=dict(mode=post.MODE_IQ, **wide), le=True, fx=(fftext.WF, None)),
            dict(zoom=9, audio=dict(mode=post.MODE_QAM, **wide)),
            dict(zoom=10, audio=dict(mode=post.MODE_SSB, **wide), nr=NR_LMS),
            dict(zoom=8, audio=dict(mode=post.MODE_SAS, **wide), fx=(fftext.INTEG, 0.1))]


# test_nr_bank_gpu.py's receiver 0 and test_nrs_bank_gpu.py's receiver 0.  `SET nr algo=` holds ONE algorithm per receiver (selecting
# NR_SPECTRAL leaves the LMS filters and the other way round), so a receiver runs the two one after the other: the script switches.
NR_LMS = (1, {1: [64, 16, 1e-4, 0.1], 0: [64, 16, 1e-4, 0.1]}, (1, 1))          # post.NR_WDSP
NR_SPECTRAL = (3, {0: [1, 0.95, 1000]}, (0, 0))                                # post.NR_SPECTRAL


def largest():
    """(b): every per-block table kind -- BL_POST, BL_NULL, BL_REAL, BL_IQ_BE, BL_IQ_LE -- staged in every sound block"""
    from flydog_sdr_gps_amd import fftext, nb, post
    wide = dict(lo=-4900.0, hi=4900.0)
    return [dict(zoom=8, audio=dict(mode=post.MODE_SSB, **wide), nb=(nb.NB_STD, [100.0, 50.0], (1, 0))),
            dict(zoom=10, audio=dict(mode=post.MODE_SAM, sam_mparam=post.CHAN_NULL_LSB, **wide), spec=2, fx=(fftext.SPEC, None)),
            dict(zoom=9, audio=dict(mode=post.MODE_IQ, **wide), le=True),
            dict(zoom=9, audio=dict(mode=post.MODE_QAM, **wide))]


@functools.lru_cache(maxsize=1)
def stream_blocks():
    """-> two int16 blocks of 2^24 samples: ONE synth.adc_stream (its carrier at 0.0123 f_adc, which the SAM PLLs lock to) with the impulse
    bursts of test_nb_bank_gpu.py's adc() added at the audio NCOs' frequency, so that both blankers act.  Made once, never written."""
    from flydog_sdr_gps_amd import synth
    n = 2 * BLOCK
    x = synth.adc_stream(n, SEED).astype(np.float32)
    for s in range(40000, n - 20000, 700001):
        x[s:s + 20000] += (26000.0 * np.sin(2 * np.pi * 0.0123 * np.arange(s, s + 20000, dtype=np.float64))).astype(np.float32)
    x = np.clip(np.round(x), -32768, 32767).astype(np.int16)
    a, b = x[:BLOCK].copy(), x[BLOCK:].copy()
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def _mix(table, n):
    from flydog_sdr_gps_amd.ddc import rx_phase_inc
    from flydog_sdr_gps_amd.rxbank import ADC_CLOCK, UI_SRATE
    from flydog_sdr_gps_amd.wf import WfParams
    hz = UI_SRATE / (1024 << 14)
    mix = []
    for k, row in enumerate(table):
        span = UI_SRATE / (1 << row["zoom"])
        p = WfParams.for_zoom(row["zoom"], (0.0123 * ADC_CLOCK - span * (0.2 + 0.07 * k)) / hz, adc_clock=ADC_CLOCK, ui_srate=UI_SRATE)
        assert 8192 * p.decim <= n, "a one-shot frame at every step size"
        mix.append((p, False, rx_phase_inc(0.0123 * ADC_CLOCK - 900.0 - 35.0 * k, ADC_CLOCK)))
    return mix


def _connect(bank, rx, row, mix, join):
    """a connection's first commands, in the order the layers ask for (set_nb / set_nr / set_spec after set_audio; the extension reads
    the mode at its command)"""
    p, ov, inc = mix[rx]
    if join:
        bank.join(rx, (p, ov), inc, **row["audio"])
    else:
        bank.set_wf(rx, p, ov)
        bank.set_audio(rx, inc, **row["audio"])
    bank.set_little_endian(rx, bool(row.get("le")))
    if "nb" in row:
        bank.set_nb(rx, *row["nb"])
    if "nr" in row:
        bank.set_nr(rx, *row["nr"])
    if "spec" in row:
        bank.set_spec(rx, row["spec"])
    if "fx" in row:
        run_, itime = row["fx"]
        if itime is not None:
            bank.fftext_set_itime(rx, itime)
        bank.fftext_set_run(rx, run_)


def run(n, steps, adc, script, rx_mode=0, table=None):
    """adc: the int16 blocks whose concatenation is the (periodic) stream; step s starts at sample s * n of it.  script: {sample position:
    [(rx, what, value)]}.  -> dict:
      "streams"  [rx][name] uint8: the concatenation over steps of exactly what each step defines (kiwigpu.h, kg_rxbank_step): raw
                 [:6 nrec], xin [:nrec], firo [:nfir], agc [:nfir] in every mode but SSB (whose AGC output goes to s16 alone: the step
                 leaves agc as it was), s16 [:nfir] and pay [:nfir / 2] in the real modes, iq_pay [:4 nfir] in the stereo ones
      "spec"     [rx] [(global block, instance, 1024 bytes)] in emission order; "fx" [rx] [(global block, bin, 1024 bytes)]
                 (global block: the receiver's snd_seq before the step + the map's blk)
      "end"      [rx] dict: fir_pos, snd_seq, squelch (3 values), fx (info bytes, ncma, sums) or None
      "steps"    per step: "info" {field: int}, "nrec" / "nfir" / "seq0" int [nrx], "blk_spec" [(rx, inst, blk)], "blk_fx" [(rx, blk)],
                 "stereo" / "le" bool [nrx], "frames" {rx: (row 1024 bytes, packet bytes)}
    """
    from flydog_sdr_gps_amd import post
    from flydog_sdr_gps_amd.rxbank import RxBank
    table = features() if table is None else table
    nrx = len(table)
    total = sum(len(b) for b in adc)
    assert total % n == 0 and all(len(b) % n == 0 or n % len(b) == 0 for b in adc)
    mix = _mix(table, n)
    mode = [row["audio"]["mode"] for row in table]
    bank = RxBank(nrx, n, rx_mode=rx_mode)
    d_adc = bank.ctx.alloc(2 * total)
    try:
        at = 0
        for b in adc:
            bank.ctx.upload(d_adc + 2 * at, b)
            at += len(b)
        bank.wf.set_tables()
        bank.fftext_set_rate(bank.fs)
        for rx, row in enumerate(table):
            _connect(bank, rx, row, mix, join=False)
        out = {"streams": [{k: [] for k in STREAMS} for _ in range(nrx)], "spec": [[] for _ in range(nrx)], "fx": [[] for _ in range(nrx)],
               "steps": []}
        for step in range(steps):
            for rx, what, v in script.get(step * n, []):
                if what == "audio":
                    bank.set_audio(rx, mix[rx][2], **v)
                    mode[rx] = v["mode"]
                elif what == "nr":
                    bank.set_nr(rx, *v)
                elif what == "leave":
                    bank.leave(rx)
                elif what == "join":
                    _connect(bank, rx, table[rx], mix, join=True)
                    mode[rx] = table[rx]["audio"]["mode"]
                elif what == "fx_clear":
                    bank.fftext_clear(rx)
                else:
                    raise KeyError(what)
            seq0 = bank.audio_map()[3].astype(np.int64)
            info = bank.step(d_adc + 2 * ((step * n) % total))
            bank.sync()
            nrec, nfir, _, _ = bank.audio_map()
            stereo = [m in post.STEREO_MODES for m in mode]
            rec = {"info": {f: int(getattr(info, f)) for f in INFO_FIELDS}, "nrec": nrec.astype(np.int64), "nfir": nfir.astype(np.int64), "seq0": seq0,
                   "stereo": list(stereo), "le": list(bank.little_endian), "frames": {}}
            live = [rx for rx in range(nrx) if nrec[rx] > 0]
            got = {k: bank.fetch(k, live) for k in STREAMS}
            for i, rx in enumerate(live):
                nr_, nf = int(nrec[rx]), int(nfir[rx])
                extent = {"raw": 6 * nr_, "xin": nr_, "firo": nf, "agc": 0 if mode[rx] == post.MODE_SSB else nf, "s16": 0 if stereo[rx] else nf, "pay": 0 if stereo[rx] else nf // 2,
                          "iq_pay": 4 * nf if stereo[rx] else 0}
                for k in STREAMS:
                    out["streams"][rx][k].append(np.ascontiguousarray(got[k][i, :extent[k]]).view(np.uint8).ravel().copy())
            rx_of, inst, blk = bank.spec_map()
            rows = bank.spec_rows()
            rec["blk_spec"] = [(int(r), int(i_), int(b_)) for r, i_, b_ in zip(rx_of, inst, blk)]
            for j, (r, i_, b_) in enumerate(rec["blk_spec"]):
                out["spec"][r].append((int(seq0[r]) + b_, i_, rows[j].tobytes()))
            rx_of, blk, bins = bank.fftext_map()
            rows = bank.fftext_rows()
            rec["blk_fx"] = [(int(r), int(b_)) for r, b_ in zip(rx_of, blk)]
            for j, (r, b_) in enumerate(rec["blk_fx"]):
                out["fx"][r].append((int(seq0[r]) + b_, int(bins[j]), rows[j].tobytes()))
            rx_of, off, nbytes = bank.frame_map()
            frows, pkts = bank.fetch("rows", list(range(len(rx_of)))), bank.fetch("pkts", list(range(len(rx_of))))
            for f, r in enumerate(rx_of):
                rec["frames"][int(r)] = (frows[f].tobytes(), pkts[f, :int(nbytes[f])].tobytes())
            out["steps"].append(rec)
        for rx in range(nrx):
            for k in STREAMS:
                out["streams"][rx][k] = np.concatenate(out["streams"][rx][k]) if out["streams"][rx][k] else np.zeros(0, np.uint8)
        _, _, pos, seq = bank.audio_map()
        fx = bank.fftext
        out["end"] = []
        for rx in range(nrx):
            sq = bank.post.squelch_state([rx])
            st = fx.state(rx, sums=True) if fx is not None else None
            out["end"].append({"fir_pos": int(pos[rx]), "snd_seq": int(seq[rx]),
                               "squelch": (int(sq[0][0]), int(sq[1][0]), sq[2].view(np.uint32)[0].item()),
                               "fx": None if st is None else (st[0].tobytes(), st[1].copy(), st[2].view(np.uint32).copy())})
        return out
    finally:
        bank.sync()
        bank.ctx.free(d_adc)
        bank.close()


def blocks(rec):
    """sound blocks per receiver of one step"""
    return (rec["nfir"] // 512).tolist()


def first_difference(long, short, nrx):
    """the first thing in which two runs differ, walking each receiver's chain in order -- or None"""
    for rx in range(nrx):
        for k in STREAMS:
            a, b = long["streams"][rx][k], short["streams"][rx][k]
            if a.size != b.size:
                return (rx, k, "bytes", a.size, b.size)
            bad = np.flatnonzero(a != b)
            if bad.size:
                return (rx, k, "first differing byte", int(bad[0]), "of", a.size, "differing", int(bad.size))
        for k in ("spec", "fx"):
            a, b = long[k][rx], short[k][rx]
            if [r[:2] for r in a] != [r[:2] for r in b]:
                return (rx, k, "row sequences (global block, instance or bin)", [r[:2] for r in a][:12], [r[:2] for r in b][:12])
            for j, (ra, rb) in enumerate(zip(a, b)):
                if ra[2] != rb[2]:
                    return (rx, k, "row", j, "global block", ra[0], "instance / bin", ra[1])
        a, b = long["end"][rx], short["end"][rx]
        for k in ("fir_pos", "snd_seq", "squelch"):
            if a[k] != b[k]:
                return (rx, "end", k, a[k], b[k])
        if (a["fx"] is None) != (b["fx"] is None):
            return (rx, "end", "fx")
        if a["fx"] is not None:
            for j, name in enumerate(("info", "ncma", "sums")):
                same = a["fx"][j] == b["fx"][j] if j == 0 else np.array_equal(a["fx"][j], b["fx"][j])
                if not same:
                    return (rx, "end", "fx " + name)
    return None
