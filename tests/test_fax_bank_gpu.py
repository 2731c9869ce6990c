"""The receiver bank's FAX extension (kg_rxbank_fax_*; extensions/FAX/FaxDecoder.cpp, fax.cpp) against a standalone kg_fax fed the bank's
own 16-bit audio (d_s16): a bank of three receivers -- rx0 in USB with FAX started, rx1 in IQ with FAX started (its blocks never go on
the mono list: it emits nothing), rx2 never started.  Records, rows and the whole end state of rx0 are equal byte for byte, through a
shift, a leave and a join (a fresh object) and a second start.  Everything else the bank hands out is byte-identical to a second bank
that is stepped the same and never told about the extension, which holds nothing for it; a bank of twice the step gives the same
lines as the short steps; FAX runs beside the IQ display and Loran-C (another tap).  A line is 1200 samples here (600 lpm at the
nominal 12 kHz): a step yields about 0.8 sound blocks, so a line completes every third step."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import FaxDecoder, KiwiGpuError, post

from . import fax_common as fc

pytestmark = pytest.mark.gpu

N = 1 << 22
NR = 3
LO, HI = -4900.0, 4900.0
USB, IQ = post.MODE_SSB, post.MODE_IQ
CFG = dict(lpm=600, imagewidth=1024, carrier=1900, deviation=400, bandwidth=1, include_headers=True, phasing=True, autostop=True, debug=0, nom_rate=12000.0)
STEPS = 30


def _bank(n=N, modes=(USB, IQ, USB)):
    from flydog_sdr_gps_amd.rxbank import MIXES, RxBank
    mix = MIXES["light"](NR, 0, N)
    bank = RxBank(NR, n)
    bank.configure(MIXES["light"](NR, 0, n))
    for rx in range(NR):
        bank.set_audio(rx, mix[rx][2], LO, HI, mode=modes[rx])
    return bank


def _state_equal(a, b, where):
    for x, y in zip(a, b):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), where


def _same_lines(got, want, where):
    assert got[0].tobytes() == want[0].tobytes(), (where, got[0], want[0])
    assert got[1].shape[0] == want[1].shape[0], where
    w = CFG["imagewidth"] + 1
    assert np.array_equal(got[1][:, :w], want[1][:, :w]), where


def test_a_bank_that_was_never_told_and_one_that_was(gpu_ctx):
    from flydog_sdr_gps_amd import live_allocs, synth
    plain, told = _bank(), _bank()
    fs = float(told.fs)
    sx = FaxDecoder(gpu_ctx, nconn=NR)
    try:
        adc = synth.adc_stream(N, 0x5EEDFA01)
        d_adc, d_adc2 = told.ctx.alloc(adc.nbytes), plain.ctx.alloc(adc.nbytes)
        told.ctx.upload(d_adc, adc)
        plain.ctx.upload(d_adc2, adc)
        assert told.fax is None and plain.fax is None and told.fax_out() == {}
        held = live_allocs()
        seen = {"lines": 0, "rows": 0, "iq_blocks": 0, "after_join": 0, "shifted": 0}
        on0 = False
        for step in range(STEPS):
            if step == 0:
                for rx in (0, 1):
                    told.fax_start(rx, srate=fs, **CFG)
                    sx.start(rx, srate=fs, **CFG)
                on0 = True
                assert live_allocs() - held == 4 and told.fax is not None      # the object's state, rows, records, counts; the slots were exchanged
            if step == 7:
                told.fax_set_shift(0, 0.4)
                sx.set_shift(0, 0.4)
            if step == 13:
                for b in (told, plain):
                    b.leave(0)
                on0 = False
                info = told.fax.state(0)[0]
                assert info["spl"] == 0 and info["started"] == 0 and info["Iprev"] == 0        # a fresh object: zeroed, not started
            if step == 15:
                for b in (told, plain):
                    b.join(0, None, None)
                    b.set_wf(0, b.params[0], b.overlapped[0])
                    b.set_audio(0, b.rx_inc[0], LO, HI, mode=USB)
                assert told.fax.state(0)[0]["spl"] == 0
            if step == 16:
                cfg = dict(CFG, lpm=500, debug=1)
                told.fax_start(0, srate=fs + 0.7, **cfg)
                fresh = FaxDecoder(gpu_ctx, nconn=NR)                          # the standalone twin of the joined receiver starts zeroed too
                sx.close()
                sx = fresh
                sx.start(0, srate=fs + 0.7, **cfg)
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
            out = told.fax_out()
            seen["iq_blocks"] += int(nfir[1]) // 512
            assert 1 not in out and 2 not in out, step                        # the IQ receiver's blocks are not on the mono list
            nblk = int(nfir[0]) // 512
            if not on0 or nblk == 0:
                assert out == {}, step
                continue
            assert list(out) == [0], step
            x = np.ascontiguousarray(s16[0, :512 * nblk]).reshape(1, nblk, 512)
            recs, rows = sx.push([0], x, [fs if step < 16 else fs + 0.7])
            _same_lines(out[0], (recs[0], rows[0]), step)
            seen["lines"] += recs[0].size
            seen["rows"] += rows[0].shape[0]
            seen["after_join"] += int(step >= 16 and recs[0].size > 0)
            seen["shifted"] += int(step >= 7 and step < 13 and recs[0].size > 0)
            if step in (12, STEPS - 1):
                _state_equal(told.fax.state(0), sx.state(0), step)
        assert seen["lines"] >= 5 and seen["rows"] >= 3 and seen["iq_blocks"] >= 8 and seen["after_join"] >= 1 and seen["shifted"] >= 1, seen
        assert told.fax.state(1)[0]["started"] == 1 and told.fax.state(1)[0]["samp_idx"] == 0      # started, never fed
        assert told.fax.state(0)[0]["lpm"] == 500                                                  # the joined receiver started afresh
        # 3. the bank that was never told holds nothing for the extension
        assert plain.fax is None and plain.fax_out() == {}
        # 4. another tap than the IQ one: FAX beside the IQ display and beside Loran-C
        told.iqd_init(0)
        told.iqd_set_run(0, 1, fs)
        told.fax_start(0, srate=fs, **CFG)
        told.lorc_init(2, fs, 600)
        told.lorc_set_gri(2, 0, 2990)
        told.lorc_set_gri(2, 1, 4970)
        told.lorc_start(2)
        told.fax_start(2, srate=fs, **CFG)
        told.step(d_adc)
        told.sync()
        assert told.iqd.state(0)[0]["run"] and told.lorc.state(2)[0]["started"] and told.fax.state(2)[0]["started"]
        # 5. what a bank refuses beyond kg_fax: fewer than 1024 samples a line, an image wider than 4096
        before = told.fax.state(2)
        with pytest.raises(KiwiGpuError):
            told.fax_start(2, srate=fs, **dict(CFG, lpm=720))
        with pytest.raises(KiwiGpuError):
            told.fax_start(2, srate=fs, **dict(CFG, lpm=60, imagewidth=4097))
        with pytest.raises(KiwiGpuError):
            told.fax_set_shift(2, -0.5)
        _state_equal(told.fax.state(2), before, "refused")
        with pytest.raises(RuntimeError):
            told.fax.push([0], np.zeros((1, 1, 512), np.int16), [fs])
        told.ctx.free(d_adc)
        plain.ctx.free(d_adc2)
    finally:
        sx.close()
        told.close()
        plain.close()


def test_a_long_step_equals_the_same_blocks_as_short_steps(gpu_ctx):
    """a bank of 2 N samples a step against one of N over the same stream: the lines of each receiver, concatenated, and the end state"""
    from flydog_sdr_gps_amd import synth
    short, long_ = _bank(N, (USB, USB, USB)), _bank(2 * N, (USB, USB, USB))
    try:
        adc = synth.adc_stream(2 * N, 0x5EEDFA02)
        half = adc.nbytes // 2
        d_s, d_l = short.ctx.alloc(adc.nbytes), long_.ctx.alloc(adc.nbytes)
        short.ctx.upload(d_s, adc)
        long_.ctx.upload(d_l, adc)
        got = {id(short): {0: [], 2: []}, id(long_): {0: [], 2: []}}
        for b in (short, long_):
            b.fax_start(0, srate=float(b.fs), **CFG)
            b.fax_start(2, srate=float(b.fs) - 1.3, **dict(CFG, lpm=700, imagewidth=640, debug=1, phasing=False))
            b.fax_set_shift(2, 0.3)

        def take(b):
            b.sync()
            for rx, (recs, rows) in b.fax_out().items():
                k = 0
                for r in recs:
                    row = b""
                    if int(r["flags"]) & fc.F_ROW_SENT:
                        row = rows[k].tobytes()
                        k += 1
                    got[id(b)][rx].append((tuple(int(r[f]) for f in fc.rec_dtype.names[1:]), row))      # all but blk: the step's own count
                assert k == rows.shape[0]

        for _ in range(8):
            long_.step(d_l)
            take(long_)
            for k in range(2):
                short.step(d_s + k * half)
                take(short)
        for rx in (0, 2):
            assert len(got[id(long_)][rx]) >= 4 and got[id(long_)][rx] == got[id(short)][rx], rx
            assert any(row for _, row in got[id(long_)][rx]), rx
            _state_equal(long_.fax.state(rx), short.fax.state(rx), rx)
        short.ctx.free(d_s)
        long_.ctx.free(d_l)
    finally:
        short.close()
        long_.close()
