"""The receiver bank's FT8 / FT4 extension (kg_rxbank_ft8_*; extensions/FT8/ft8_lib) against a stand-alone kg_ft8 fed the bank's own 16-bit
audio (d_s16): a bank of three receivers -- rx0 in USB with FT4 started, rx1 in IQ with it started (its blocks never go on the mono
list: it is never fed), rx2 never started.  Events, the slot record of the slot end and the whole end state of rx0 -- schedule,
last_frame, both waterfalls -- are equal byte for byte, under a clock that moves every step.  Everything else the bank hands out is
byte-identical to a second bank that is stepped the same and never told about the extension, which holds nothing for it.  A bank of
twice the step gives the same events, slot record and state as the short steps, and steps enqueued with no wait the same as awaited
ones.  FT8 refuses FAX and the CW decoder on one receiver and they refuse it (the real-samples tap holds one task); leave and join give a
fresh, uninitialised connection."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import Ft8, KiwiGpuError, ft8, post

pytestmark = pytest.mark.gpu

N = 1 << 24                                         # about three sound blocks a step: an FT4 slot (148 blocks of 576 samples) ends near the 54th
NR = 3
LO, HI = -4900.0, 4900.0
USB, IQ = post.MODE_SSB, post.MODE_IQ
T0, DT = 7500.8125, 0.14                            # the first step syncs; the clock is an input and need not follow the samples
STEPS = 60
FAX_CFG = dict(lpm=600, imagewidth=1024, nom_rate=12000.0)


def _bank(n=N, modes=(USB, IQ, USB)):
    from flydog_sdr_gps_amd.rxbank import MIXES, RxBank
    mix = MIXES["light"](NR, 0, n)
    bank = RxBank(NR, n)
    bank.configure(mix)
    for rx in range(NR):
        bank.set_audio(rx, mix[rx][2], LO, HI, mode=modes[rx])
    return bank


def whole_state(q, c):
    info, lf, mag = q.state(c)
    return [info.tobytes(), lf.tobytes(), mag.tobytes(), q.state(c, previous=True)[2].tobytes()]


def test_a_bank_that_was_never_told_and_one_that_was(gpu_ctx):
    from flydog_sdr_gps_amd import synth
    plain, told = _bank(), _bank()
    sx = Ft8(gpu_ctx, nconn=NR)
    try:
        adc = synth.adc_stream(N, 0x5EEDF801)
        d_adc, d_adc2 = told.ctx.alloc(adc.nbytes), plain.ctx.alloc(adc.nbytes)
        told.ctx.upload(d_adc, adc)
        plain.ctx.upload(d_adc2, adc)
        told.ft8_set_now(5.0)                                                # a clock alone makes nothing
        assert told.ft8 is None and plain.ft8 is None and told.ft8_out()[1] == {}
        with pytest.raises(KiwiGpuError):
            told.ft8_start(0)                                                # before init
        for rx in (0, 1):
            told.ft8_init(rx, ft8.FT4)
            told.ft8_start(rx)
            sx.init(rx, ft8.FT4)
        seen = {"events": 0, "slots": 0, "blocks": 0, "iq_blocks": 0}
        for step in range(STEPS):
            now = T0 + DT * step
            told.ft8_set_now(now)
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
            # 2. the stand-alone object on the bank's own audio
            evs, slots = told.ft8_out()
            seen["iq_blocks"] += int(nfir[1]) // 512
            assert not (set(evs["conn"].tolist()) | set(slots)) - {0}, step    # the IQ receiver's blocks are not on the mono list
            nblk = int(nfir[0]) // 512
            if nblk == 0:
                assert evs.size == 0 and not slots, step
                continue
            x = np.ascontiguousarray(s16[0, :512 * nblk]).reshape(1, nblk, 512)
            ev2, sl2 = sx.push([0], x, now)
            assert evs.tobytes() == ev2.tobytes(), (step, evs, ev2)
            assert len(slots) == sl2.size and (not slots or slots[0].tobytes() == sl2[0].tobytes()), (step, "the slot record")
            seen["events"] += evs.size
            seen["slots"] += len(slots)
            seen["blocks"] += nblk
            if slots or step == STEPS - 1:
                assert whole_state(told.ft8, 0) == whole_state(sx, 0), step
        print("seen", seen)
        assert seen["slots"] == 1 and seen["events"] == 3 and seen["iq_blocks"] >= 150, seen      # a sync, the slot end, the next sync
        info1 = told.ft8.state(1)[0]
        assert info1["inited"] == 1 and info1["tsync"] == 0 and info1["slot"] == 0             # started, never fed
        # 3. the bank that was never told holds nothing for the extension
        plain.ft8_stop(0)                                                    # a stop makes nothing either
        assert plain.ft8 is None and plain.ft8_out()[1] == {}
        # 4. the real-samples tap holds one task: FT8, FAX and the CW decoder refuse each other on one receiver, whoever came first
        fs = float(told.fs)
        before = whole_state(told.ft8, 0)
        for call in (lambda: told.fax_start(0, srate=fs, **FAX_CFG), lambda: told.cw_start(0, 40, 12000.0, fs)):
            with pytest.raises(KiwiGpuError):
                call()
        assert whole_state(told.ft8, 0) == before
        told.fax_start(2, srate=fs, **FAX_CFG)
        told.ft8_init(2, ft8.FT8)
        with pytest.raises(KiwiGpuError):
            told.ft8_start(2)
        told.fax_stop(2)
        told.cw_start(2, 40, 12000.0, fs)
        with pytest.raises(KiwiGpuError):
            told.ft8_start(2)
        told.cw_stop(2)
        told.ft8_start(2)                                                    # ... and takes the tap once they have let go of it
        told.ft8_stop(0)
        told.fax_start(0, srate=fs, **FAX_CFG)
        told.fax_stop(0)
        # 5. leave and join: a fresh connection, not initialised, last_frame zeroed
        told.ft8_start(0)
        told.leave(0)
        info, lf, mag = told.ft8.state(0)
        assert info["inited"] == 0 and info["slot"] == 0 and not lf.any()
        told.join(0, None, None)
        told.set_wf(0, told.params[0], told.overlapped[0])
        told.set_audio(0, told.rx_inc[0], LO, HI, mode=USB)
        with pytest.raises(KiwiGpuError):
            told.ft8_start(0)
        told.ft8_init(0, ft8.FT8)
        told.ft8_start(0)
        told.ft8_set_now(15000.8125)
        told.step(d_adc)
        told.sync()
        evs, slots = told.ft8_out()
        assert [(int(e["conn"]), int(e["kind"]), int(e["a"])) for e in evs] == [(0, ft8.EV_SLOT_START, 1), (2, ft8.EV_SLOT_START, 1)] and not slots
        assert told.ft8.state(0)[0]["nfft"] == 3840 and told.ft8.state(0)[0]["in_pos"] >= 1024
        # 6. refusals pass through unchanged, and the bank's object is fed by its steps alone
        for call in (lambda: told.ft8_init(0, 2), lambda: told.ft8_init(0, ft8.FT8, 20250.0), lambda: told.ft8_init(NR, 0), lambda: told.ft8_start(NR),
                     lambda: told.ft8_set_now(float("nan")), lambda: told.ft8_set_now(-1.0)):
            with pytest.raises(KiwiGpuError):
                call()
        with pytest.raises(RuntimeError):
            told.ft8.push([0], np.zeros((1, 1, 512), np.int16), 0.0)
        told.ctx.free(d_adc)
        plain.ctx.free(d_adc2)
    finally:
        sx.close()
        told.close()
        plain.close()


def test_long_steps_and_steps_with_no_wait_equal_short_awaited_steps(gpu_ctx):
    """a bank of 2 N samples a step, and a bank of N whose steps are enqueued with no wait up to the slot end, against one of N that is
    waited for every step, over the same stream with the clock moving every long step: the events (all but the block of the step), the
    slot record and the end state of both receivers, one FT4 and one FT8"""
    from flydog_sdr_gps_amd import synth
    short, nowait, long_ = _bank(N, (USB, USB, USB)), _bank(N, (USB, USB, USB)), _bank(2 * N, (USB, USB, USB))
    try:
        adc = synth.adc_stream(2 * N, 0x5EEDF802)
        half = adc.nbytes // 2
        d = {}
        for b in (short, nowait, long_):
            d[id(b)] = b.ctx.alloc(adc.nbytes)
            b.ctx.upload(d[id(b)], adc)
            b.ft8_init(0, ft8.FT4)
            b.ft8_init(2, ft8.FT8)
            b.ft8_start(0)
            b.ft8_start(2)
        got = {id(b): dict(ev=[], slots=[]) for b in (short, nowait, long_)}

        def take(b):
            b.sync()
            evs, slots = b.ft8_out()
            got[id(b)]["ev"] += [tuple(int(e[f]) for f in ("conn", "kind", "a", "b", "t")) for e in evs]
            got[id(b)]["slots"] += [(rx, s.tobytes()) for rx, s in sorted(slots.items())]

        end_at = None
        for k in range(30):
            for b in (short, nowait, long_):
                b.ft8_set_now(T0 + 2 * DT * k)
            long_.step(d[id(long_)])
            take(long_)
            for h in range(2):
                short.step(d[id(short)] + h * half)
                take(short)
                if got[id(short)]["slots"] and end_at is None:
                    end_at = (k, h)
        assert end_at is not None and len(got[id(short)]["slots"]) == 1 and got[id(short)]["slots"][0][0] == 0
        for k in range(30):                                                  # the same steps with no wait between them, up to the one that ends the slot
            nowait.ft8_set_now(T0 + 2 * DT * k)
            for h in range(2):
                nowait.step(d[id(nowait)] + h * half)
                if (k, h) == end_at:
                    take(nowait)
        nowait.sync()
        assert got[id(long_)]["ev"] == got[id(short)]["ev"] and len(got[id(short)]["ev"]) >= 4
        assert got[id(long_)]["slots"] == got[id(short)]["slots"] == got[id(nowait)]["slots"]
        for rx in (0, 2):
            want = whole_state(short.ft8, rx)
            assert whole_state(long_.ft8, rx) == want and whole_state(nowait.ft8, rx) == want, rx
        assert short.ft8.state(2)[0]["num_blocks"] >= 30 and short.ft8.state(2)[0]["nfft"] == 3840
        for b in (short, nowait, long_):
            b.ctx.free(d[id(b)])
    finally:
        short.close()
        nowait.close()
        long_.close()
