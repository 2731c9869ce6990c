"""The receiver bank's WSPR extension (kg_rxbank_wspr_*; extensions/wspr/) against a standalone kg_wspr fed the bank's own CFastFIR
output, with int_decimate 1 (snd_rate 375) and long steps so that a cycle end is reached: rx0 captures from an even minute on, rx1
free-running from an odd one with more_candidates and type 15 and a passage through NBFM (where it gets nothing), rx2 is initialised and
never captures.  Rows, row map, events, cycle ends, counts and the whole end state -- planes and samples -- are equal byte for byte.
Everything else the bank hands out is byte-identical to a second bank that is stepped the same and never told about the extension,
which holds nothing for it; a bank of twice the step gives the same rows as the short steps; ten steps enqueued with no wait give what
ten awaited steps give; the IQ tap's one callback goes to the IQ display, to Loran-C or to WSPR, never to two; leave and join give a
fresh object."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import KiwiGpuError, post, wspr

pytestmark = pytest.mark.gpu

N = 1 << 22
NR = 3
LO, HI = -4900.0, 4900.0
USB, NBFM = post.MODE_SSB, post.MODE_NBFM
STEPS = 18                                      # of 8 N: 6.4 sound blocks a step; group 85 is due in the 87th block


def _bank(n):
    from flydog_sdr_gps_amd.rxbank import MIXES, RxBank
    mix = MIXES["light"](NR, 0, N)
    bank = RxBank(NR, n)
    bank.configure(MIXES["light"](NR, 0, n))
    for rx in range(NR):
        bank.set_audio(rx, mix[rx][2], LO, HI, mode=USB)
    return bank


def _state(w, rx):
    info, avg, planes, iq = w.state(rx, planes=True, samples=True)
    return info.tobytes(), avg.tobytes(), planes.tobytes(), iq.tobytes()


def _rows_of(m, rows, packed):
    """(receiver, block, sample, group, half, sync flag, the 412 bytes) per row; packed: rows [n, 412], else the byte array of push()"""
    return [(int(r["conn"]), int(r["blk"]), int(r["samp"]), int(r["group"]), int(r["half"]), int(r["tsync"]),
             (rows[i] if packed else rows[int(r["off"]):int(r["off"]) + 412]).tobytes()) for i, r in enumerate(m)]


def test_a_bank_that_was_never_told_and_one_that_was(gpu_ctx):
    from flydog_sdr_gps_amd import synth
    n = 8 * N
    plain, told = _bank(n), _bank(n)
    sx = wspr.Wspr(gpu_ctx, nconn=NR)
    try:
        adc = synth.adc_stream(n, 0x5EED0F2A)
        d_adc, d_adc2 = told.ctx.alloc(adc.nbytes), plain.ctx.alloc(adc.nbytes)
        told.ctx.upload(d_adc, adc)
        plain.ctx.upload(d_adc2, adc)
        assert told.wspr is None and plain.wspr is None
        for w, who in ((told, lambda f: getattr(told, "wspr_" + f)), (sx, lambda f: getattr(sx, f))):
            who("init")(0, 375.0)
            who("set_capture")(0, 1)
            who("init")(2, 375.0)
        assert told.wspr is not None
        mode, on = {rx: USB for rx in range(NR)}, {0: True, 1: False, 2: False}
        seen = {"rows0": 0, "rows1": 0, "nbfm1": 0, "ends": 0, "sync": 0}
        clock = (0, 0)
        for step in range(STEPS):
            if step == 1:
                clock = (1, 7)                                            # an odd minute: rx1 runs free, rx0 is not synchronised again
            if step == 2:
                for who in (lambda f: getattr(told, "wspr_" + f), lambda f: getattr(sx, f)):
                    who("init")(1, 375.0)
                    who("set_type")(1, 15)
                    who("set_more_candidates")(1, 1)
                    who("set_capture")(1, 1)
                on[1] = True
            if step in (5, 6):
                for b in (told, plain):
                    b.post.set_mode(1, NBFM if step == 5 else USB)
                mode[1] = NBFM if step == 5 else USB
            told.wspr_set_now(*clock)
            told.step(d_adc)
            plain.step(d_adc2)
            told.sync()
            plain.sync()
            maps, maps2 = [np.array(m).copy() for m in told.audio_map()], [np.array(m).copy() for m in plain.audio_map()]
            for a, b in zip(maps, maps2):                                 # 1. nothing else changes
                assert np.array_equal(a, b), step
            nfir = maps[1]
            out, out2 = ({k: b.fetch(k, list(range(NR))) for k in ("firo", "s16")} for b in (told, plain))
            for rx in range(NR):
                for k in ("firo", "s16"):
                    m = int(nfir[rx])
                    assert np.array_equal(np.ascontiguousarray(out[k][rx, :m]).view(np.uint8), np.ascontiguousarray(out2[k][rx, :m]).view(np.uint8)), (step, rx, k)
            # 2. the standalone object on the bank's own filter output
            firo = np.ascontiguousarray(out["firo"]).view(np.complex64).reshape(NR, -1)
            fed = [rx for rx in range(NR) if on[rx] and mode[rx] != NBFM and int(nfir[rx]) >= 512]
            seen["nbfm1"] += int(on[1] and mode[1] == NBFM and int(nfir[1]) >= 512)
            rows_got, m_got, ev_got, cyc_got, cnt_got = told.wspr_out()
            if not fed:
                assert m_got.size == 0 and ev_got.size == 0, step
                continue
            nblk = [int(nfir[rx]) // 512 for rx in fed]
            host = np.zeros((len(fed), max(nblk), 512), np.complex64)
            for i, rx in enumerate(fed):
                host[i, :nblk[i]] = firo[rx, :512 * nblk[i]].reshape(-1, 512)
            rows, m, ev, cyc, counts = sx.push(fed, host, clock[0], clock[1], nblk=nblk)
            assert _rows_of(m_got, rows_got, True) == _rows_of(m, rows, False), step
            assert ev_got.tobytes() == ev.tobytes(), (step, ev_got, ev)
            assert sorted(cyc_got) == [rx for i, rx in enumerate(fed) if cyc[i]["due"]], step
            for i, rx in enumerate(fed):
                assert cnt_got[rx].tobytes() == counts[i].tobytes(), (step, rx)
                if cyc[i]["due"]:
                    assert cyc_got[rx].tobytes() == cyc[i].tobytes(), (step, rx)
                    assert wspr.messages(ev_got, cyc_got) == wspr.messages(ev, cyc, conns=fed)
            assert 2 not in m_got["conn"]
            seen["rows0"] += int((m["conn"] == 0).sum())
            seen["rows1"] += int((m["conn"] == 1).sum())
            seen["ends"] += len(cyc_got)
            seen["sync"] += int(m["tsync"].sum())
        for rx in range(NR):
            assert _state(told.wspr, rx) == _state(sx, rx), rx
        # the walk met every case: both receivers' rows, the NBFM step, a cycle end of each reached in long steps, and the sync flag of rx0's
        # group 0 -- twice: all blocks of a step carry one time, so the first step's 0:00 synchronises rx0 at its first block and, re-armed
        # at group 3 (:767), again at its sixth
        assert seen["rows0"] >= 86 and seen["rows1"] >= 60 and seen["nbfm1"] == 1 and seen["ends"] == 2 and seen["sync"] == 2, seen
        assert told.wspr.state(0)[0]["cycles"] == 1 and told.wspr.state(1)[0]["wspr_type"] == 15
        # 3. the bank that was never told holds nothing for the extension
        assert plain.wspr is None and plain.wspr_out()[1].size == 0
        # 4. the tap holds one callback: the IQ display, Loran-C or WSPR
        fs = told.fs
        for rx in (0, 1):
            told.iqd_init(rx)
            with pytest.raises(KiwiGpuError):
                told.iqd_set_run(rx, 1, fs)
            told.lorc_init(rx, float(fs), 600)
            told.lorc_set_gri(rx, 0, 2990)
            told.lorc_set_gri(rx, 1, 2990)
            with pytest.raises(KiwiGpuError):
                told.lorc_start(rx)
        assert not told.iqd.state(0)[0]["run"] and not told.lorc.state(0)[0]["started"] and told.wspr.state(0)[0]["capture"] == 1
        told.iqd_init(2)
        told.iqd_set_run(2, 1, fs)
        before = _state(told.wspr, 2)
        with pytest.raises(KiwiGpuError):
            told.wspr_set_capture(2, 1)
        assert _state(told.wspr, 2) == before and told.wspr.state(2)[0]["capture"] == 0
        told.iqd_set_run(2, 0, fs)
        told.lorc_init(2, float(fs), 600)
        told.lorc_set_gri(2, 0, 2990)
        told.lorc_set_gri(2, 1, 2990)
        told.lorc_start(2)
        with pytest.raises(KiwiGpuError):
            told.wspr_set_capture(2, 1)
        told.lorc_stop(2)
        told.wspr_set_capture(2, 1)
        told.wspr_set_capture(0, 0)
        told.iqd_set_run(0, 1, fs)                                        # capture off gave the tap back
        with pytest.raises(KiwiGpuError):
            told.wspr_set_now(60, 0)
        # 5. leave and join: a fresh object, zeroed, not initialised, not capturing
        told.leave(1)
        told.join(1, None, None)
        info, avg, planes, iq = told.wspr.state(1, planes=True, samples=True)
        assert not info["inited"] and not info["capture"] and not info["didx"] and not avg.any() and not planes.any() and not iq.any()
        with pytest.raises(KiwiGpuError):
            told.wspr_set_capture(1, 1)                                   # before its `SET ext_server_init`
        told.ctx.free(d_adc)
        plain.ctx.free(d_adc2)
    finally:
        sx.close()
        told.close()
        plain.close()


def _start(b):
    b.wspr_init(0, 375.0)
    b.wspr_set_capture(0, 1)
    b.wspr_init(2, 750.0)
    b.wspr_set_more_candidates(2, 1)
    b.wspr_set_capture(2, 1)


def test_a_long_step_equals_the_same_blocks_as_short_steps(gpu_ctx):
    """a bank of 8 N samples a step against one of 4 N over the same stream: the rows of each receiver, concatenated, the events and the
    end state.  The first long step and the first two short ones stand at 0:00 (the sync), the rest at an odd minute"""
    from flydog_sdr_gps_amd import synth
    short, long_ = _bank(4 * N), _bank(8 * N)
    try:
        adc = synth.adc_stream(8 * N, 0x5EED0F2B)
        half = adc.nbytes // 2
        d_s, d_l = short.ctx.alloc(adc.nbytes), long_.ctx.alloc(adc.nbytes)
        short.ctx.upload(d_s, adc)
        long_.ctx.upload(d_l, adc)
        got = {id(short): {0: [], 2: []}, id(long_): {0: [], 2: []}}
        evs = {id(short): [], id(long_): []}
        for b in (short, long_):
            _start(b)

        def take(b):
            b.sync()
            rows, m, ev, cyc, counts = b.wspr_out()
            for r in _rows_of(m, rows, True):
                got[id(b)][r[0]].append(r[3:])                             # group, half, flag, bytes: the block of a step differs by design
            evs[id(b)] += [(int(e["conn"]), int(e["kind"]), int(e["a"]), int(e["b"])) for e in ev]

        for k in range(5):
            for b in (short, long_):
                b.wspr_set_now(*((0, 0) if k == 0 else (1, 30)))
            long_.step(d_l)
            take(long_)
            for h in range(2):
                short.step(d_s + h * half)
                take(short)
        for rx in (0, 2):
            assert len(got[id(long_)][rx]) >= (24 if rx == 0 else 12) and got[id(long_)][rx] == got[id(short)][rx], rx
            assert _state(long_.wspr, rx) == _state(short.wspr, rx), rx
        assert sorted(evs[id(long_)]) == sorted(evs[id(short)]) and len(evs[id(long_)]) == 7       # IDLE, SYNC and the sync's RUNNING of two receivers, and rx0's second sync at 0:00 behind its re-arm
        assert got[id(long_)][0][0][2] == 1                                # group 0 of the synchronised cycle carries the flag
        short.ctx.free(d_s)
        long_.ctx.free(d_l)
    finally:
        short.close()
        long_.close()


def test_ten_steps_enqueued_with_no_wait_equal_the_stepwise_ones(gpu_ctx):
    """the host runs ahead: ten steps, a command and a new clock between them with no wait against the same steps awaited one by one --
    every step's row map and events (the host's), the last step's rows and the end state"""
    from flydog_sdr_gps_amd import synth
    wait, deep = _bank(4 * N), _bank(4 * N)
    try:
        adc = synth.adc_stream(4 * N, 0x5EED0F2C)
        d_w, d_d = wait.ctx.alloc(adc.nbytes), deep.ctx.alloc(adc.nbytes)
        wait.ctx.upload(d_w, adc)
        deep.ctx.upload(d_d, adc)
        maps = {id(wait): [], id(deep): []}
        for b, d, awaited in ((wait, d_w, True), (deep, d_d, False)):
            _start(b)
            b.wspr_set_now(1, 59)
            b.step(d)                                                     # the first step of a bank drains by design
            b.sync()
            for k in range(10):
                if k == 3:
                    b.wspr_set_now(2, 0)                                  # the even minute: both receivers synchronise in this step
                if k == 4:
                    b.wspr_set_now(2, 1)
                if k == 5:
                    b.wspr_set_type(0, 15)                                # a command between two enqueued steps: host state only
                b.step(d)
                if awaited:
                    b.sync()
                m, ev = np.zeros(256, wspr.row_dtype), np.zeros(64, wspr.ev_dtype)
                import ctypes as C
                n, ne = C.c_int32(), C.c_int32()
                assert b.lib.kg_rxbank_wspr_out(b.h, None, None, None, m.ctypes.data_as(C.c_void_p), 256, C.byref(n), ev.ctypes.data_as(C.c_void_p), 64, C.byref(ne),
                                                None, 0) == 2
                maps[id(b)].append((m[:n.value].tobytes(), ev[:ne.value].tobytes()))
            b.sync()
        assert maps[id(wait)] == maps[id(deep)] and sum(len(m) for m, e in maps[id(wait)]) >= 20 * 32 and sum(len(e) for m, e in maps[id(wait)]) == 2 * 24
        rw, mw = wait.wspr_out()[:2]
        rd, md = deep.wspr_out()[:2]
        assert _rows_of(mw, rw, True) == _rows_of(md, rd, True) and mw.size >= 2
        for rx in (0, 2):
            assert _state(wait.wspr, rx) == _state(deep.wspr, rx), rx
        wait.ctx.free(d_w)
        deep.ctx.free(d_d)
    finally:
        wait.close()
        deep.close()
