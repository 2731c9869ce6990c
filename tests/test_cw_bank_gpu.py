"""The receiver bank's CW decoder extension (kg_rxbank_cw_*; extensions/CW_decoder/uhsdr_cw_decoder.cpp, cw_decoder.cpp) against a
standalone kg_cw fed the bank's own 16-bit audio (d_s16): a bank of three receivers -- rx0 in USB with the decoder started, rx1 in IQ
with it started (its blocks never go on the mono list: it emits nothing), rx2 never started.  Events and the whole end state of rx0 are
equal byte for byte, through a pboff, a leave and a join (a fresh object) and a second start, under a clock that moves every step.
Everything else the bank hands out is byte-identical to a second bank that is stepped the same and never told about the extension,
which holds nothing for it; a bank of twice the step gives the same events as the short steps; the decoder and FAX refuse each other on
one receiver (the real-samples tap holds one task), run on two different receivers of one bank, and the decoder runs beside the IQ
display; a first use whose allocations are refused one after the other leaves the bank as it was.  The audio is the noise of the
synthetic ADC stream under a low threshold: marks and spaces of a few Goertzel blocks, which train, decode and fail as any keying
does."""
import gc

import numpy as np
import pytest

from flydog_sdr_gps_amd import Context, CwDecoder, KiwiGpuError, cw, live_allocs, post

pytestmark = pytest.mark.gpu

N = 1 << 22
NR = 3
LO, HI = -4900.0, 4900.0
USB, IQ = post.MODE_SSB, post.MODE_IQ
NOM = 12000.0
THRESHOLD = 300
STEPS = 30
FAX_CFG = dict(lpm=600, imagewidth=1024, nom_rate=NOM)


def _bank(n=N, modes=(USB, IQ, USB)):
    from flydog_sdr_gps_amd.rxbank import MIXES, RxBank
    mix = MIXES["light"](NR, 0, N)
    bank = RxBank(NR, n)
    bank.configure(MIXES["light"](NR, 0, n))
    for rx in range(NR):
        bank.set_audio(rx, mix[rx][2], LO, HI, mode=modes[rx])
    return bank


def _tell(q, rx, fs, ti=40, pboff=818, bank=True, threshold=THRESHOLD):
    """the client's first commands, on a bank or on a standalone object"""
    if bank:
        q.cw_start(rx, ti, NOM, fs)
        q.cw_set_pboff(rx, pboff)
        q.cw_set_threshold(rx, threshold)
    else:
        q.start(rx, ti, NOM, fs)
        q.set_pboff(rx, pboff)
        q.set_threshold(rx, threshold)


def _median_magnitude(s16, bin_):
    """the median Goertzel magnitude of whole 88-sample blocks of the audio at a bin: a threshold there makes noise key the decoder"""
    x = s16[:s16.size // 88 * 88].astype(np.float64).reshape(-1, 88) / 4
    return int(np.median(np.abs(x @ np.exp(-2j * np.pi * bin_ * np.arange(88) / 88))))


def test_a_bank_that_was_never_told_and_one_that_was(gpu_ctx):
    from flydog_sdr_gps_amd import synth
    plain, told = _bank(), _bank()
    fs = float(told.fs)
    sx = CwDecoder(gpu_ctx, nconn=NR)
    try:
        adc = synth.adc_stream(N, 0x5EEDC301)
        d_adc, d_adc2 = told.ctx.alloc(adc.nbytes), plain.ctx.alloc(adc.nbytes)
        told.ctx.upload(d_adc, adc)
        plain.ctx.upload(d_adc2, adc)
        told.cw_set_now(5)                                                   # a clock alone makes nothing
        assert told.cw is None and plain.cw is None and told.cw_out() == {}
        warm = []
        while sum(w.size for w in warm) < 2 * 512:                           # the threshold is an input: where this audio's noise lies
            for b in (told, plain):
                b.step(d_adc if b is told else d_adc2)
                b.sync()
            warm.append(told.fetch("s16", [0])[0, :int(told.audio_map()[1][0])].copy())
        thr = _median_magnitude(np.concatenate(warm), 6)
        assert thr >= 1
        held = live_allocs()
        seen = {"events": 0, "kinds": set(), "iq_blocks": 0, "after_join": 0, "fed": 0}
        on0 = False
        for step in range(STEPS):
            now = 1000 + 3 * step
            told.cw_set_now(now)
            if step == 0:
                for rx in (0, 1):
                    _tell(told, rx, fs, threshold=thr)
                    _tell(sx, rx, fs, bank=False, threshold=thr)
                on0 = True
                assert live_allocs() - held == 3 and told.cw is not None      # the object's state, events, counts; the slots were exchanged
            if step == 7:
                told.cw_set_pboff(0, 1200)
                sx.set_pboff(0, 1200)
            if step == 13:
                for b in (told, plain):
                    b.leave(0)
                on0 = False
                assert not np.frombuffer(told.cw.state(0).tobytes(), np.uint8).any()      # a fresh object: zeroed, not started, slowdown with it
            if step == 15:
                for b in (told, plain):
                    b.join(0, None, None)
                    b.set_wf(0, b.params[0], b.overlapped[0])
                    b.set_audio(0, b.rx_inc[0], LO, HI, mode=USB)
                assert told.cw.state(0)["blocksize"] == 0
            if step == 16:
                _tell(told, 0, fs + 0.7, ti=20, pboff=700, threshold=thr)
                fresh = CwDecoder(gpu_ctx, nconn=NR)                           # the standalone twin of the joined receiver starts zeroed too
                sx.close()
                sx = fresh
                _tell(sx, 0, fs + 0.7, ti=20, pboff=700, bank=False, threshold=thr)
                on0 = True
            told.step(d_adc)
            plain.step(d_adc2)
            told.sync()
            plain.sync()
            # 1. nothing else changes
            maps, maps2 = told.audio_map(), plain.audio_map()
            for a, b in zip(maps, maps2):
                assert np.array_equal(a, b), step
            nfir = maps[1]
            s16, s16b = told.fetch("s16", list(range(NR))), plain.fetch("s16", list(range(NR)))
            pay, payb = told.fetch("pay", list(range(NR))), plain.fetch("pay", list(range(NR)))
            for rx in range(NR):
                n = int(nfir[rx])
                assert np.array_equal(s16[rx, :n], s16b[rx, :n]) and np.array_equal(pay[rx, :n // 2], payb[rx, :n // 2]), (step, rx)
            # 2. the standalone object on the bank's own audio
            out = told.cw_out()
            seen["iq_blocks"] += int(nfir[1]) // 512
            assert 1 not in out and 2 not in out, step                        # the IQ receiver's blocks are not on the mono list
            nblk = int(nfir[0]) // 512
            if not on0 or nblk == 0:
                assert out == {}, step
                continue
            assert list(out) == [0], step
            x = np.ascontiguousarray(s16[0, :512 * nblk]).reshape(1, nblk, 512)
            evs = sx.push([0], x, [now])[0]
            assert out[0].tobytes() == evs.tobytes(), (step, out[0], evs)
            seen["events"] += evs.size
            seen["kinds"] |= set(evs["kind"].tolist())
            seen["fed"] += 1
            seen["after_join"] += int(step >= 16 and evs.size > 0)
            if step in (12, STEPS - 1):
                assert told.cw.state(0).tobytes() == sx.state(0).tobytes(), step
        st0 = told.cw.state(0)
        print("seen", seen, "threshold", thr, "ring", int(st0["sig_lastrx"]), "dot", float(st0["dot_avg"]), "dash", float(st0["dash_avg"]), "old_siglevel", float(st0["old_siglevel"]))
        assert seen["events"] >= 100 and {cw.PLOT, cw.TRAIN} <= seen["kinds"] and seen["iq_blocks"] >= 8 and seen["after_join"] >= 1 and seen["fed"] >= 8, seen
        assert told.cw.state(0)["sig_lastrx"] >= 1                                                   # the noise keyed the ring
        assert told.cw.state(1)["started"] == 1 and told.cw.state(1)["sample_counter"] == 0 and told.cw.state(1)["slowdown"] == 0      # started, never fed
        assert told.cw.state(0)["training_interval"] == 20 and told.cw.state(0)["g_a"] == cw_bin(700, fs + 0.7)      # the joined receiver started afresh
        # 3. the bank that was never told holds nothing for the extension
        assert plain.cw is None and plain.cw_out() == {}
        # 4. the real-samples tap holds one task: the decoder and FAX refuse each other on one receiver, whoever came first
        before = told.cw.state(0).tobytes()
        with pytest.raises(KiwiGpuError):
            told.fax_start(0, srate=fs, **FAX_CFG)
        assert told.cw.state(0).tobytes() == before and told.fax.state(0)[0]["started"] == 0 and told.fax.state(0)[0]["spl"] == 0
        told.fax_start(2, srate=fs, **FAX_CFG)
        with pytest.raises(KiwiGpuError):
            told.cw_start(2, 40, NOM, fs)
        assert told.cw.state(2)["blocksize"] == 0 and told.cw.state(2)["started"] == 0
        # ... run on two different receivers of one bank, the decoder beside the IQ display
        told.iqd_init(0)
        told.iqd_set_run(0, 1, fs)
        fed = {0: 0, 2: 0}
        for _ in range(4):
            told.step(d_adc)
            told.sync()
            fed[0] += int(0 in told.cw_out())
            fed[2] += int(2 in told.fax_out())
            assert 2 not in told.cw_out() and 0 not in told.fax_out()
        assert fed[0] >= 2 and fed[2] >= 2 and told.iqd.state(0)[0]["run"] and told.cw.state(0)["started"] and told.fax.state(2)[0]["started"]
        # ... and each takes the tap once the other has let go of it
        told.cw_stop(0)
        told.fax_start(0, srate=fs, **FAX_CFG)
        told.fax_stop(2)
        told.cw_start(2, 40, NOM, fs)
        # 5. refusals pass through unchanged, and the bank's object is fed by its steps alone
        before = told.cw.state(2).tobytes()
        for call in (lambda: told.cw_start(2, 0, NOM, fs), lambda: told.cw_set_pboff(2, 6100), lambda: told.cw_set_wpm(2, -1, 40), lambda: told.cw_start(NR, 40, NOM, fs),
                     lambda: told.cw_start(2, 40, NOM, float("nan"))):
            with pytest.raises(KiwiGpuError):
                call()
        assert told.cw.state(2).tobytes() == before
        with pytest.raises(RuntimeError):
            told.cw.push([0], np.zeros((1, 1, 512), np.int16), [0])
        told.ctx.free(d_adc)
        plain.ctx.free(d_adc2)
    finally:
        sx.close()
        told.close()
        plain.close()


def cw_bin(pboff, srate):
    """g->a (uhsdr_cw_decoder.cpp:299) in the reference's operand types"""
    f = np.float32
    return int(0.5 + float(f(f(f(pboff) * f(88)) / f(srate))))


def test_a_long_step_equals_the_same_blocks_as_short_steps(gpu_ctx):
    """a bank of 2 N samples a step against one of N over the same stream, the clock moving every long step: the events of each receiver,
    concatenated, and the end state"""
    from flydog_sdr_gps_amd import synth
    short, long_ = _bank(N, (USB, USB, USB)), _bank(2 * N, (USB, USB, USB))
    try:
        adc = synth.adc_stream(2 * N, 0x5EEDC302)
        half = adc.nbytes // 2
        d_s, d_l = short.ctx.alloc(adc.nbytes), long_.ctx.alloc(adc.nbytes)
        short.ctx.upload(d_s, adc)
        long_.ctx.upload(d_l, adc)
        got = {id(short): {0: [], 2: []}, id(long_): {0: [], 2: []}}
        for b in (short, long_):
            _tell(b, 0, float(b.fs))
            _tell(b, 2, float(b.fs) - 1.3, ti=25, pboff=1000)
            b.cw_set_auto_threshold(2, 1)
            b.cw_set_threshold(2, THRESHOLD // 2)

        def take(b):
            b.sync()
            for rx, evs in b.cw_out().items():
                got[id(b)][rx] += [tuple(int(e[f]) for f in cw.ev_dtype.names[1:]) for e in evs]      # all but blk: the step's own count

        for k in range(8):
            for b in (short, long_):
                b.cw_set_now(500 + 5 * k)
            long_.step(d_l)
            take(long_)
            for h in range(2):
                short.step(d_s + h * half)
                take(short)
        for rx in (0, 2):
            assert len(got[id(long_)][rx]) >= 40 and got[id(long_)][rx] == got[id(short)][rx], rx
            assert long_.cw.state(rx).tobytes() == short.cw.state(rx).tobytes(), rx
        assert long_.cw.state(2)["isAutoThreshold"] == 1 and long_.cw.state(2)["threshold_linear"] == THRESHOLD // 2
        short.ctx.free(d_s)
        long_.ctx.free(d_l)
    finally:
        short.close()
        long_.close()


def test_a_failed_first_use_leaves_the_bank_as_it_was(monkeypatch):
    """the RxBank.fax case of tests/test_lifecycle_gpu.py for the CW decoder: every allocation of the first use -- the grown slots, pinned
    and on the device, the events, the counts, the object's state -- is refused once; the call that finally works, and the same call
    again, give what a bank that never saw a refusal gives, and nothing stays allocated"""
    from .test_lifecycle_gpu import CREATES, as_bytes, bank_ext, prep_bank, refused_until_it_works

    def tell(b):
        b.cw_set_now(77)
        _tell(b, 0, float(b.fs))

    call = bank_ext(tell, lambda b: [[rx, evs] for rx, evs in sorted(b.cw_out().items())])
    create = CREATES["RxBank"][0]
    gc.collect()
    live0 = live_allocs()

    def fresh():
        c = Context(0)
        o = create(c)
        prep_bank(o)
        return c, o

    ctx, obj = fresh()
    first, refusals = refused_until_it_works(monkeypatch, lambda: call(obj), 64)
    assert refusals >= 4
    again = call(obj)
    assert first[0] and first[0][0][0] == 0 and first[0][0][1].size >= 1          # receiver 0 was fed on the last step, which completed a sound block
    obj.close()
    ctx.close()
    assert live_allocs() == live0
    ctx, obj = fresh()
    want = [as_bytes(call(obj)), as_bytes(call(obj))]
    obj.close()
    ctx.close()
    assert [as_bytes(first), as_bytes(again)] == want
    assert live_allocs() == live0
